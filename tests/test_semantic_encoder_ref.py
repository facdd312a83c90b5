"""C12h on the CPU: the torch restatement of the semantic encoder (tests/semantic_encoder_ref.py) against HuggingFace's own HubertModel + nn.LSTM + nn.Linear,
through the fixtures tools/make_hf_golden.py wrote (`hubert` mode; transformers is not imported here) - every tap within 1e-4 of the tap's largest magnitude,
both sides f32, and HF's id on every decided frame; the frame-count formula; the 24 kHz -> 16 kHz resampler of bark.cpp_amd/voice.py."""
import importlib.util
import os

import numpy as np
import pytest

import semantic_encoder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _voice():
    spec = importlib.util.spec_from_file_location("bark_voice_for_resampler", os.path.join(ROOT, "bark.cpp_amd", "voice.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def toy():
    from tools.make_synth_hubert import ensure_hubert
    return ref.load(ensure_hubert("hub_toy", 0)), np.load(os.path.join(ROOT, "tests", "golden", "hf_hub_toy_s0.npz"))


@pytest.mark.parametrize("n", ref.TOY_LENGTHS)
def test_restatement_matches_hf_at_every_tap(toy, n):
    (hp, W), g = toy
    taps, ids = ref.encode(hp, W, ref.fixture_signal(n))
    for name in ref.TAPS:
        got, want = taps[name], g[f"{name}_n{n}"]
        if name == "conv0" and f"tap0_rows_n{n}" in g.files:
            got = got[g[f"tap0_rows_n{n}"]]
        assert got.shape == want.shape, name
        dev, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"n={n} {name}: {dev:.2e} of {scale:.2f}")
        assert dev <= 1e-4 * scale, (name, dev, scale)
    decided = g[f"margin_n{n}"] > 8.0 * float(g[f"logits_f16emu_maxabs_n{n}"])
    assert ids.shape == (ref.frame_count(n),) and np.array_equal(ids[decided], g[f"ids_n{n}"][decided])


def test_fixture_conditions_hold(toy):
    """what the GPU tests rely on, re-read from the fixtures: at 16000 samples at least 8 distinct ids and at least half of the frames decided"""
    for g in (toy[1], np.load(os.path.join(ROOT, "tests", "golden", "hf_hub_base_s0.npz"))):
        ids = g["ids_n16000"]
        decided = g["margin_n16000"] > 8.0 * float(g["logits_f16emu_maxabs_n16000"])
        assert len(ids) == 49 and len(set(ids.tolist())) >= 8 and 2 * int(decided.sum()) >= len(ids)
        m, top = g["margin_n16000"], g["top2_n16000"]
        assert (m >= 0).all() and np.array_equal(top[:, 0], ids)


def test_frame_count_formula(toy):
    (hp, W), _ = toy
    with pytest.raises(ValueError):
        ref.frame_count(399)
    assert [ref.frame_count(n) for n in (400, 719, 720, 16000, 48000, 328079)] == [1, 1, 2, 49, 149, 1024]
    assert ref.frame_count(328080) == 1025
    for n in (400, 719, 720):                             # the seven valid convolutions give the same count
        assert len(ref.encode(hp, W, ref.fixture_signal(n))[1]) == ref.frame_count(n)
    with pytest.raises(Exception):
        ref.encode(hp, W, ref.fixture_signal(399))


def test_f16_mode_moves_the_taps_by_about_what_hf_moves(toy):
    """the reference's f16 mode is the measure the head test takes its bound from: it must be of the size HF's own f16 emulation shows"""
    (hp, W), g = toy
    x = ref.fixture_signal(1040)
    a, _ = ref.encode(hp, W, x)
    b, _ = ref.encode(hp, W, x, f16=True)
    for name in ref.TAPS:
        mine, hf = float(np.abs(a[name] - b[name]).max()), float(g[f"{name}_f16emu_maxabs_n1040"])
        assert 0.25 * hf <= mine <= 4.0 * hf, (name, mine, hf)


def test_resampler_length_and_sine():
    v = _voice()
    for n in (0, 1, 2, 3, 4, 100, 101, 24000, 24001):
        assert len(v.resample_24k_to_16k(np.zeros(n, np.float32))) == -(-2 * n // 3), n
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(24000) / 24000.0).astype(np.float32)
    y = v.resample_24k_to_16k(x)
    want = np.sin(2.0 * np.pi * 1000.0 * np.arange(16000) / 16000.0)
    assert y.dtype == np.float32 and float(np.abs(y - want)[32:-32].max()) < 1e-3
    # above the new Nyquist frequency nothing passes
    hi = np.sin(2.0 * np.pi * 10000.0 * np.arange(24000) / 24000.0).astype(np.float32)
    assert float(np.abs(v.resample_24k_to_16k(hi))[32:-32].max()) < 1e-2
