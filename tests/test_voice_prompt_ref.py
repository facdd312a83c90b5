"""CPU tests of rule C10v (voice prompts) and of its restatement tests/voice_prompt_ref.py - the yardstick the GPU tests of
tests/test_gpu_voice_prompts.py hold the engine to.  Two things pin the restatement before it judges anything:
  1. with an EMPTY history its three loops reproduce Oracle.coarse / Oracle.fine / Oracle.generate id for id (greedy and seeded);
  2. under the HF numerics (set_numerics(False, tanh)) it reproduces HuggingFace's own `generate(history_prompt=...)` id for id on three synthetic
     histories (tests/golden/hf_toy_voice_s0.npz, written by `tools/make_hf_golden.py voice`)."""
import os

import numpy as np
import pytest

from tests import voice_prompt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hf_toy_voice_s0.npz")
TEXT = "hello world , the water is cold today and the river runs fast !"


def test_empty_history_is_the_oracle_greedy(toy_oracle):
    o = toy_oracle
    p = o.params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=150)
    sem = o.semantic(o.tokenize(TEXT), p)
    assert np.array_equal(R.semantic(o, o.tokenize(TEXT), None, n_steps=150), sem)
    co = o.coarse(sem, p)
    assert len(co) > 120                                           # several windows, the history cap not yet reached
    assert np.array_equal(R.coarse(o, sem, None), co)
    assert np.array_equal(R.fine(o, co, None), o.fine(co, p))
    # non-default window parameters: history cap active, odd window count
    p2 = o.params(temp=0.0, fine_temp=0.0, sliding_window_size=30, max_coarse_history=100)
    assert np.array_equal(R.coarse(o, sem, None, sliding_window_size=30, max_coarse_history=100), o.coarse(sem, p2))


def test_empty_history_is_the_oracle_over_two_fine_windows(toy_oracle):
    rng = np.random.default_rng(5)
    co = rng.integers(0, 1024, (1100, 2)).astype(np.int32)
    want = toy_oracle.fine(co, toy_oracle.params(temp=0.0, fine_temp=0.0))
    assert np.array_equal(R.fine(toy_oracle, co, None), want)


def test_empty_history_is_the_oracle_seeded(toy_oracle):
    o = toy_oracle
    o.seed(7)
    want = o.generate("hello world", o.params(temp=0.7, fine_temp=0.5, n_steps_text_encoder=40))
    got = R.generate(o, "hello world", None, temp=0.7, fine_temp=0.5, n_steps=40, seed=7)
    for k in ("semantic", "coarse", "fine", "pcm"):
        assert np.array_equal(got[k], want[k]), k


def test_trim_rule_on_the_stated_cases():
    # short: n_sem odd, floor(2 Tc / r) the smallest term and odd -> the kept coarse history starts on the SECOND codebook
    v = R.synthetic_voice(1, 35, 41, 41)
    hs, hc = R.trim(v)
    assert len(hs) == 27 and len(hc) == 81 - 2
    assert np.array_equal(hs, v.semantic[-27:])
    flat = (v.coarse + 10000 + 1024 * np.arange(2)[None, :]).reshape(-1)
    assert np.array_equal(hc, flat[-81:-2]) and 11024 <= hc[0] < 12048
    # full: every cap active
    hs, hc = R.trim(R.synthetic_voice(2, 300, 700, 700))
    assert len(hs) == 209 and len(hc) == 628 - 2
    # a smaller history cap
    hs, hc = R.trim(R.synthetic_voice(2, 300, 700, 700), max_coarse_history=100)
    assert len(hs) == 33 and len(hc) == 99 - 2
    for n_sem, tc in ((1, 41), (35, 1), (3, 1)):                  # n_sh < 2 or n_ch <= 2: python's x[-0:] would take the whole array
        with pytest.raises(ValueError):
            R.trim(R.synthetic_voice(3, n_sem, tc, 10))
    assert [len(x) for x in R.trim(None)] == [0, 0]


def test_semantic_prompt_rule():
    base = np.concatenate([np.arange(256) + 10048, np.full(256, 10000), [129599]]).astype(np.int32)
    v = R.synthetic_voice(4, 300, 50, 50)
    p = R.semantic_prompt(base, v)
    assert np.array_equal(p[:256], base[:256]) and p[512] == 129599 and np.array_equal(p[256:512], v.semantic[-256:])
    v = R.synthetic_voice(4, 35, 50, 50)
    p = R.semantic_prompt(base, v)
    assert np.array_equal(p[256:291], v.semantic) and (p[291:512] == 10000).all()
    assert np.array_equal(R.semantic_prompt(base, None), base)


def test_fine_window_plan():
    # no history: today's plan (bark.cpp:1998-2013)
    assert R.fine_windows(0, 100) == ([(0, 0, 0)], 1024)
    assert R.fine_windows(0, 1100) == ([(0, 0, 0), (76, 512, 436)], 1100)
    # rel == n_hist on the full windows, larger on a short last one
    assert R.fine_windows(512, 100) == ([(0, 512, 512)], 1024)
    assert R.fine_windows(512, 1100) == ([(0, 512, 512), (512, 1024, 512), (588, 1100, 512)], 1612)
    assert R.fine_windows(100, 1100) == ([(0, 100, 100), (176, 612, 436)], 1200)
    assert R.fine_windows(41, 1052) == ([(0, 41, 41), (69, 553, 484)], 1093)
    for n_hist, T in ((0, 1), (41, 60), (512, 513), (100, 924), (100, 925), (512, 8192)):
        wins, L = R.fine_windows(n_hist, T)
        filled = np.zeros(L, bool)
        for start, fill, rel in wins:
            assert 0 <= start and start + 1024 <= L and fill >= n_hist and 0 <= rel < 1024
            filled[fill:fill + 1024 - rel] = True
        assert filled[n_hist:n_hist + T].all() and not filled[:n_hist].any()


@pytest.mark.parametrize("name", ["short", "full", "tf100"])
def test_voice_loops_against_hf_generate_with_history_prompt(toy_oracle, name):
    """HuggingFace's BarkSemanticModel / BarkCoarseModel / BarkFineModel .generate(history_prompt=...) against voice_prompt_ref over the oracle's
    evaluations in HF-matching numerics: id for id (as test_stage_loops_against_hf_generate does without a history)."""
    g = np.load(GOLD)
    o = toy_oracle
    v = R.Voice(g[f"{name}_h_semantic"], g[f"{name}_h_coarse"], g[f"{name}_h_fine"])
    try:
        o.set_numerics(act_round_f16=False, gelu_mode=1)
        t = g["text_ids"].astype(np.int64)
        prompt = np.concatenate([t + 10048, np.full(256 - len(t), 129595), np.full(256, 10000), [129599]]).astype(np.int32)
        got_s = R.semantic(o, prompt, v, min_eos_p=2.0, n_steps=int(g["n_semantic_steps"]))
        assert np.array_equal(got_s, g[f"{name}_semantic_from_text"]), "semantic ids differ from HF generate"
        got_c = R.coarse(o, g["semantic"], v)
        want_c = g[f"{name}_coarse"]
        assert got_c.shape == want_c.shape, (got_c.shape, want_c.shape)
        assert np.array_equal(got_c, want_c), f"coarse ids differ from HF generate, first at row {int(np.flatnonzero((got_c != want_c).any(axis=1))[0])}"
        want_f = g[f"{name}_fine"]
        assert len(R.fine_windows(min(len(v.fine), 512), len(want_c))[0]) >= 2
        got_f = R.fine(o, want_c, v)
        assert got_f.shape == want_f.shape and np.array_equal(got_f, want_f), "fine ids differ from HF generate"
    finally:
        o.set_numerics(act_round_f16=True, gelu_mode=0)


def test_voice_file_round_trip_and_npz_layout(tmp_path):
    from bark_amd_loader import load_package
    voice = load_package().voice
    src = R.synthetic_voice(9, 123, 77, 55)
    v = voice.VoicePrompt(src.semantic, src.coarse, src.fine)
    path = str(tmp_path / "speaker.bvp")
    voice.save(v, path)
    assert os.path.getsize(path) == 16 + 4 * (123 + 2 * 77 + 8 * 55)
    raw = open(path, "rb").read()
    assert raw[:4] == b"BVP1" and np.array_equal(np.frombuffer(raw, "<i4", 3, 4), [123, 77, 55])
    assert voice.load(path) == v
    # Suno's presets are codebook-major
    npz = str(tmp_path / "speaker.npz")
    np.savez(npz, semantic_prompt=src.semantic, coarse_prompt=src.coarse.T, fine_prompt=src.fine.T)
    assert voice.from_npz(npz) == v
    open(path, "wb").write(raw[:-4])
    with pytest.raises(ValueError):
        voice.load(path)
    open(path, "wb").write(b"XXXX" + raw[4:])
    with pytest.raises(ValueError):
        voice.load(path)
