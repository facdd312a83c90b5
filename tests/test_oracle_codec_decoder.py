"""The CPU oracle's EnCodec decoder (oracle/bark_oracle.cpp: codec_decode) pinned independently of the engine: (a) the numpy restatement
tests/codec_decoder_ref.py against the four committed HuggingFace fixtures, (b) the oracle in HF-matching numerics against the restatement, PCM and all
six taps, at the lengths where the padding rule takes its short-input detour (T <= 2 at the K = 3 residual convolutions, T <= 6 at the K = 7 first one)
and at every codebook depth the GPU tests use, (c) the same inputs in the default numerics, (d) the condition that keeps (b) from being blind to the
detour.  No GPU.  Bounds: 2e-5 of scale in HF-matching numerics and 5e-3 in the default ones, as tests/test_oracle_golden.py states them."""
import os

import numpy as np
import pytest

import codec_decoder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 2, 3, 6, 7, 33, 65)
DEPTHS = {"toy": (1, 2, 8), "mini": (1, 2, 8), "small": (1, 2, 8, 32)}
HF_BOUND, DEFAULT_BOUND = 2e-5, 5e-3


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


def codes_for(preset, n_q, T):
    """the code matrix of a case: one seeded draw per (preset, n_q, T)"""
    seed = 1000 * ("toy", "mini", "small").index(preset) + 40 * T + n_q
    return np.random.default_rng(seed).integers(0, 1024, (n_q, T)).astype(np.int32)


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
def restated():
    """(pcm, taps) of the restatement per case, computed once and shared by (b) and (c)"""
    tens, done = {}, {}

    def tensors(preset):
        if preset not in tens:
            tens[preset] = ref.codec_tensors(_model(preset))[1]
        return tens[preset]

    def get(preset, n_q, T):
        if (preset, n_q, T) not in done:
            pcm, taps = ref.decode(tensors(preset), codes_for(preset, n_q, T))
            pcm.setflags(write=False)
            for t in taps:
                t.setflags(write=False)
            done[(preset, n_q, T)] = (pcm, taps)
        return done[(preset, n_q, T)]
    get.tensors = tensors
    return get


def _rel(got, want):
    got = np.asarray(got, np.float64).reshape(-1); want = np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,preset,T", [("hf_toy_s0.npz", "toy", 3), ("hf_toy_s0.npz", "toy", 50), ("hf_small_codec_s0.npz", "small", 5),
                                              ("hf_small_codec_s0.npz", "small", 40)], ids=lambda v: str(v))
def test_restatement_matches_the_hf_fixtures(restated, fixture, preset, T):
    """HF's own EncodecDecoder on the same tensors.  Measured: 5.9e-7 to 1.3e-6 of full scale."""
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    pcm, _ = ref.decode(restated.tensors(preset), g[f"codec_codes_T{T}"])
    err = _rel(pcm, g[f"codec_pcm_T{T}"])
    print(f"{preset} T={T}: max |restatement - HF| / scale = {err:.2e}")
    assert err <= HF_BOUND


# ---- (b), (c) -----------------------------------------------------------------------------------------------------------------------------------------
def _oracle_against_restatement(orc, restated, preset, T):
    """max over the depths of the relative deviation (each tap against its own maximum): {'pcm': e, 'tap0': e, ...}"""
    worst = {}
    for n_q in DEPTHS[preset]:
        codes = codes_for(preset, n_q, T)
        pcm, taps = restated(preset, n_q, T)
        errs = {"pcm": _rel(orc.codec_decode(codes), pcm)}
        for st in range(6):
            errs[f"tap{st}"] = _rel(orc.codec_tap(codes, st), taps[st])
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


CASES = [(p, T) for p in ("toy", "mini", "small") for T in LENGTHS]


@pytest.mark.parametrize("preset,T", CASES, ids=lambda v: str(v))
def test_hf_matching_oracle_equals_the_restatement_at_every_tap(oracles, restated, preset, T):
    """act_round_f16 off, erf GELU: both sides compute in f32 over the same tensors.  T <= 2: the K = 3 convolutions take _pad1d's detour; T <= 6: the
    K = 7 ones; 7 is the first length without it.  Measured over all cases: <= 2.1e-6 (PCM), <= 1.9e-6 (taps)."""
    orc = oracles(preset)
    orc.set_numerics(act_round_f16=False, gelu_mode=2)
    try:
        worst = _oracle_against_restatement(orc, restated, preset, T)
    finally:
        orc.set_numerics(act_round_f16=True, gelu_mode=0)
    print(f"{preset} T={T} n_q in {DEPTHS[preset]}, HF-matching numerics: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert max(worst.values()) <= HF_BOUND, worst


@pytest.mark.parametrize("preset,T", CASES, ids=lambda v: str(v))
def test_default_oracle_stays_within_f16_noise_of_the_restatement(oracles, restated, preset, T):
    """The numerics the engine is held to bit for bit (f16-rounded activations in front of every product, C9m): they must differ from f32, and by
    rounding noise only.  Measured: 6.6e-4 to 1.2e-3 of scale (PCM), 2.1e-4 to 9.2e-4 (taps, each against its own maximum)."""
    orc = oracles(preset)
    orc.set_numerics(act_round_f16=True, gelu_mode=0)
    orc.set_codec_mfma(True)
    worst = _oracle_against_restatement(orc, restated, preset, T)
    print(f"{preset} T={T} n_q in {DEPTHS[preset]}, default numerics: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    assert 0 < worst["pcm"] <= DEFAULT_BOUND, worst
    assert all(0 < e <= DEFAULT_BOUND for e in worst.values()), worst


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["toy", "mini", "small"])
@pytest.mark.parametrize("T", [1, 2])
def test_the_short_input_detour_is_visible(restated, preset, T):
    """A decoder whose padding skips the zero-extension (reflection where it is defined, the edge value otherwise) must miss the true PCM by more than
    100 times the bound of (b) - otherwise (b) could not tell whether the oracle takes the detour."""
    codes = codes_for(preset, 8, T)
    pcm, _ = restated(preset, 8, T)
    wrong, _ = ref.decode(restated.tensors(preset), codes, pad=ref.pad1d_without_extension)
    err = _rel(wrong, pcm)
    print(f"{preset} T={T}: a decoder without the detour deviates by {err:.2e} of scale")
    assert err > 100 * HF_BOUND
