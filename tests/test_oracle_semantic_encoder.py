"""The CPU oracle's semantic encoder (oracle/bark_oracle.cpp: semantic_encode, hub_head - rule C12h restated in scalar C++) pinned without a GPU, so that the
bit-exact GPU tests (tests/test_gpu_semantic_encoder_oracle.py) compare the engine with something that is itself held: (a) against the torch restatement
tests/semantic_encoder_ref.py (pinned to HuggingFace by tests/test_semantic_encoder_ref.py) within the reference's own sensitivity to the engine's number
formats, (b) against the committed HuggingFace fixtures, (c) on the signals that have no fixture, (d) the condition under which bit equality with a device is
decidable - no canonical transcendental of any input of the GPU tests lies next to the midpoint of two floats -, and (e) its pick on exact ties.  The host-emulated
engine is held to the oracle bit for bit by tests/test_emulated_semantic_encoder.py."""
import os

import numpy as np
import pytest

import semantic_encoder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = {name: i for i, name in enumerate(ref.TAPS)}
REF_LENGTHS = tuple(sorted(set(ref.TOY_LENGTHS) | {n for n in ref.ORACLE_S1 if ref.frame_count(n) <= 129}))


def _hubert(preset):
    from tools.make_synth_hubert import ensure_hubert
    return ensure_hubert(preset, 0)


@pytest.fixture(scope="module")
def oracles():
    from oracle.pyoracle import Oracle
    from tools.make_synth_model import ensure_model
    cache = {}

    def get(preset, path=None):
        key = path or preset
        if key not in cache:
            o = Oracle(ensure_model("toy", 0), n_threads=8)
            o.load_semantic_encoder(path or _hubert(preset))
            cache[key] = o
        return cache[key]
    yield get
    for o in cache.values():
        o.close()


@pytest.fixture(scope="module")
def weights():
    cache = {}

    def get(preset):
        if preset not in cache:
            cache[preset] = ref.load(_hubert(preset))
        return cache[preset]
    return get


def _decided_ids_equal(ids, want_ids, margin, logits_bound):
    decided = margin > 8.0 * logits_bound
    assert np.array_equal(ids[decided], want_ids[decided]), (np.flatnonzero(decided & (ids != want_ids))[:4], ids[decided][:8], want_ids[decided][:8])
    return int(decided.sum())


def test_loading_and_refusals(oracles, toy_oracle):
    orc = oracles("hub_toy")
    assert orc.has_semantic_encoder() and not toy_oracle.has_semantic_encoder()
    hp = ref.load(_hubert("hub_toy"))[0]
    assert orc.semantic_hparams() == {k: hp[k] for k in ref.HPARAM_NAMES}
    x = ref.fixture_signal(1040)
    good = orc.semantic_encode(x)
    assert good.shape == (3,) and good.dtype == np.int32
    with pytest.raises(RuntimeError):
        toy_oracle.semantic_encode(x)
    with pytest.raises(RuntimeError):
        toy_oracle.load_semantic_encoder(os.path.join(ROOT, "tests", "golden", "hf_hub_toy_s0.npz"))      # not an encoder file
    for bad_n in (399, 328080):
        with pytest.raises(RuntimeError):
            orc.semantic_encode(np.zeros(bad_n, np.float32))
    for bad in (np.nan, np.inf, -np.inf, 65520.0, -1e5):              # the engine's door: a sample that is not finite, or whose f16 image is not
        y = x.copy(); y[500] = bad
        with pytest.raises(RuntimeError):
            orc.semantic_encode(y)
    with pytest.raises(RuntimeError):
        orc.semantic_encode_tap(x, 6)
    with pytest.raises(RuntimeError):
        orc.semantic_head(np.zeros((1025, hp["H"]), np.float32))
    assert np.array_equal(orc.semantic_encode(x), good)
    assert len(orc.semantic_encode(np.zeros(328079, np.float32))) == 1024


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", REF_LENGTHS, ids=lambda v: f"n{v}_")
def test_oracle_against_the_torch_reference_at_every_tap(oracles, weights, n):
    """hub_toy at the fixture lengths and at every frame-count edge of the GPU tests up to 129 frames.  Bound per tap: 4 x max|ref(f16=True) - ref(f16=False)| +
    1e-5, the project's bound for the device (tests/test_gpu_semantic_encoder.py), computed from the reference alone; ids equal on every frame whose reference
    margin exceeds 8 x the logits' bound."""
    hp, W = weights("hub_toy")
    x = ref.oracle_signal(n)
    want, want_ids = ref.encode(hp, W, x)
    emu, _ = ref.encode(hp, W, x, f16=True)
    got, ids = oracles("hub_toy").semantic_encode_taps(x)
    worst, bounds = [], {}
    for name in ref.TAPS:
        allowed = 4.0 * float(np.abs(emu[name] - want[name]).max()) + 1e-5
        g = got[STAGE[name]]
        dev = float(np.abs(g - want[name]).max()) if g.shape == want[name].shape else np.inf
        print(f"hub_toy n={n} tap {STAGE[name]} ({name}): measured {dev:.3e} allowed {allowed:.3e}")
        worst.append((name, g.shape, want[name].shape, dev, allowed)); bounds[name] = allowed
    for name, gs, ws, dev, allowed in worst:
        assert gs == ws and dev <= allowed, (name, gs, ws, dev, allowed)
    margin, _ = ref.margins(want["logits"])
    k = _decided_ids_equal(ids, want_ids, margin, (bounds["logits"] - 1e-5) / 4.0)
    print(f"hub_toy n={n}: {k} of {len(ids)} frames decided")
    assert ids.shape == (ref.frame_count(n),)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------
HF_CASES = [("hub_toy", n) for n in ref.TOY_LENGTHS] + [("hub_base", n) for n in ref.BASE_LENGTHS]


@pytest.mark.parametrize("preset,n", HF_CASES, ids=[f"{p}-n{n}_" for p, n in HF_CASES])
def test_oracle_against_the_hf_fixtures(oracles, preset, n):
    """The comparison tests/test_gpu_semantic_encoder.py makes for the device, made for the oracle: every tap the fixture holds (hub_toy: all six; hub_base:
    hidden_states[7] alone - its taps 3 and 5 go against the torch reference in the next test) within 4 x f16emu_maxabs + 1e-5, ids HF's on every decided frame."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"hf_{preset}_s0.npz"))
    x = ref.fixture_signal(n)
    stages = tuple(STAGE[name] for name in ref.TAPS if f"{name}_n{n}" in g.files)
    assert stages == ((0, 1, 2, 3, 4, 5) if preset == "hub_toy" else (4,))
    got, ids = oracles(preset).semantic_encode_taps(x, (0, 1, 2, 3, 4, 5) if preset == "hub_toy" else (3, 4, 5))
    worst = []
    for st in stages:
        name = ref.TAPS[st]
        a, want = got[st], g[f"{name}_n{n}"]
        if name == "conv0" and f"tap0_rows_n{n}" in g.files:
            a = a[g[f"tap0_rows_n{n}"]]
        allowed = 4.0 * float(g[f"{name}_f16emu_maxabs_n{n}"]) + 1e-5
        dev = float(np.abs(a - want).max()) if a.shape == want.shape else np.inf
        print(f"{preset} n={n} tap {st} ({name}): measured {dev:.3e} allowed {allowed:.3e}")
        worst.append((name, a.shape, want.shape, dev, allowed))
    for name, gs, ws, dev, allowed in worst:
        assert gs == ws and dev <= allowed, (name, gs, ws, dev, allowed)
    k = _decided_ids_equal(ids, g[f"ids_n{n}"], g[f"margin_n{n}"], float(g[f"logits_f16emu_maxabs_n{n}"]))
    print(f"{preset} n={n}: {k} of {len(ids)} frames decided, {int((ids == g[f'ids_n{n}']).sum())} equal HF's")
    if preset == "hub_base":
        # taps 3 and 5 have no HF values in this fixture (test_oracle_at_hubert_base_widths_against_the_torch_reference holds them): shapes, finite, ids = their argmax
        assert got[3].shape == (len(ids), 768) and got[5].shape == (len(ids), 10000) and np.isfinite(got[3]).all() and np.isfinite(got[5]).all()
        assert np.array_equal(ids, np.argmax(got[5], axis=1))


def test_oracle_at_hubert_base_widths_against_the_torch_reference(oracles, weights):
    """hub_base, taps 3 - 5 and the ids at 16000 samples against the torch restatement (the HF fixture of hub_base holds hidden_states[7] only): the bound of (a)."""
    hp, W = weights("hub_base")
    x = ref.fixture_signal(16000)
    want, want_ids = ref.encode(hp, W, x)
    emu, _ = ref.encode(hp, W, x, f16=True)
    got, ids = oracles("hub_base").semantic_encode_taps(x, (3, 4, 5))
    bounds = {}
    for st in (3, 4, 5):
        name = ref.TAPS[st]
        bounds[name] = 4.0 * float(np.abs(emu[name] - want[name]).max()) + 1e-5
        dev = float(np.abs(got[st] - want[name]).max())
        print(f"hub_base n=16000 tap {st} ({name}): measured {dev:.3e} allowed {bounds[name]:.3e}")
        assert got[st].shape == want[name].shape and dev <= bounds[name], (name, dev, bounds[name])
    _decided_ids_equal(ids, want_ids, ref.margins(want["logits"])[0], (bounds["logits"] - 1e-5) / 4.0)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------------
NO_FIXTURE = [(kind, ref.ORACLE_S2_N) for kind in ref.ORACLE_S2_SIGNALS] + [ref.ORACLE_S3[0]]


@pytest.mark.parametrize("kind,n", NO_FIXTURE, ids=[f"{k}-n{n}_" for k, n in NO_FIXTURE])
def test_signals_without_a_fixture(oracles, weights, kind, n):
    """All zeros (variance exactly 0), a constant 0.5 (the clamp of the variance), +1 / -1 alternating (the largest convolution-0 outputs) at 5200 samples, and the
    1024-frame signal of the stale-scratch test: no value is non-finite at any tap, and the ids are the torch reference's on every decided frame."""
    hp, W = weights("hub_toy")
    x = ref.oracle_signal(n, kind)
    stages = (1, 2, 3, 4, 5) if n >= ref.ORACLE_LONG else (0, 1, 2, 3, 4, 5)
    got, ids = oracles("hub_toy").semantic_encode_taps(x, stages)
    for st in stages:
        assert np.isfinite(got[st]).all(), (kind, st)
    want, want_ids = ref.encode(hp, W, x)
    emu, _ = ref.encode(hp, W, x, f16=True)
    bound = float(np.abs(emu["logits"] - want["logits"]).max())
    k = _decided_ids_equal(ids, want_ids, ref.margins(want["logits"])[0], bound)
    print(f"{kind} n={n}: {k} of {len(ids)} frames decided; logits deviate {float(np.abs(got[5] - want['logits']).max()):.3e}, allowed {4.0 * bound + 1e-5:.3e}")
    assert float(np.abs(got[5] - want["logits"]).max()) <= 4.0 * bound + 1e-5


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------------------
def _census_cases():
    cases = [("hub_toy", "fixture", n, True) for n in ref.ORACLE_S1]
    cases += [("hub_toy", kind, ref.ORACLE_S2_N, True) for kind in ref.ORACLE_S2_SIGNALS]
    cases += [("hub_toy", kind, n, True) for kind, n in ref.ORACLE_S3]
    cases += [("hub_toy", "fixture", n, False) for n in ref.ORACLE_S4_LENGTHS]             # mask 1024: the convolutions in order C9
    cases += [("hub_base", "fixture", n, True) for n in ref.ORACLE_S6]
    return sorted(set(cases))


@pytest.mark.parametrize("preset,kind,n,mfma", _census_cases(), ids=lambda v: str(v))
def test_no_transcendental_of_a_gpu_test_input_lies_next_to_a_float_midpoint(oracles, preset, kind, n, mfma):
    """gelu_erf_canon and the LSTM's gate functions round a double-precision libm value to f32 once; the device's libm may differ from the host's in the last
    place of the double, which can change the f32 only next to the midpoint of two floats.  The oracle counts the values within 8 double-ulps of one
    (Oracle.near_midpoints); for every (preset, signal, length, convolution order) the GPU tests use the count is zero along the whole path.  Per value the
    chance is about 3e-8 and a 1024-frame input forms 2e7 values, so seed 0 misses the condition at some lengths: ref.ORACLE_SEEDS names the first seed that
    meets it there (hub_toy: 41040 and 41360 seed 1, 327759 seed 1, 327760 seed 2 - in both convolution orders; hub_base 48000: seed 4)."""
    orc = oracles(preset)
    orc.set_codec_mfma(mfma)
    try:
        orc.semantic_encode(ref.oracle_signal(n, kind, preset))
        count = orc.near_midpoints()
    finally:
        orc.set_codec_mfma(True)
    assert count == 0, (preset, kind, n, mfma, count)


def test_the_census_counts_what_it_should(oracles):
    """The counter is not blind: seed 0 at 327759 samples forms one erf GELU value 6 double-ulps from the midpoint of two floats (the reason that length runs on
    seed 1), and every call starts its own count."""
    orc = oracles("hub_toy")
    orc.semantic_encode(ref.fixture_signal(327759, 0))
    assert orc.near_midpoints() >= 1
    orc.semantic_encode(ref.oracle_signal(400))
    assert orc.near_midpoints() == 0                                   # every call starts its own count


@pytest.mark.parametrize("T", ref.ORACLE_S5_T, ids=lambda v: f"T{v}_")
def test_head_rows_meet_the_condition_and_the_reference(oracles, weights, T):
    hp, W = weights("hub_toy")
    feats = ref.head_rows(T, hp["H"])
    ids, logits = oracles("hub_toy").semantic_head(feats)
    assert oracles("hub_toy").near_midpoints() == 0
    want, want_ids = ref.head(hp, W, feats)
    emu, _ = ref.head(hp, W, feats, f16=True)
    bound = 4.0 * float(np.abs(emu - want).max()) + 1e-5
    dev = float(np.abs(logits - want).max())
    print(f"head T={T}: measured {dev:.3e} allowed {bound:.3e}")
    assert logits.shape == want.shape and dev <= bound
    sure = ref.margins(want)[0] > 2.0 * bound
    assert np.array_equal(ids[sure], want_ids[sure])
    assert np.array_equal(ids, np.argmax(logits, axis=1))
    if T >= 63:
        assert len(set(ids.tolist())) > T // 8


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_head_answers_the_lower_id_of_two_equal_classes(oracles, weights, tmp_path):
    """The tie file of the GPU test (ref.write_tie_hubert on ref.tie_pairs): the rows do tie - equal logits in every frame, the pair holds the row's maximum in at
    least one frame - and the oracle answers the lower id, never the higher, for the neighbour pair and for the pair 64 classes apart."""
    hp, W = weights("hub_toy")
    feats = ref.head_rows(129, hp["H"])
    base_ids = ref.head(hp, W, feats)[1]
    pairs = ref.tie_pairs(base_ids, hp["n_classes"])
    path = str(tmp_path / "hubert_toy_ties.bin")
    ref.write_tie_hubert(_hubert("hub_toy"), path, pairs)
    W2 = ref.load(path)[1]
    orc = oracles(None, path)
    ids, logits = orc.semantic_head(feats)
    assert orc.near_midpoints() == 0
    for lo, hi, src in pairs:
        assert src in (lo, hi) and (base_ids == src).sum() >= 2
        assert np.array_equal(W2["head.out.weight"][lo], W2["head.out.weight"][hi]) and W2["head.out.bias"][lo] == W2["head.out.bias"][hi]
        assert np.array_equal(logits[:, lo], logits[:, hi])
        top = logits.max(axis=1)
        assert (logits[:, lo] == top).any()
        assert not (ids == hi).any() and (ids == lo).any()
        assert np.array_equal(ids[logits[:, lo] == top], np.full(int((logits[:, lo] == top).sum()), lo))
