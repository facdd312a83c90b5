"""The semantic encoder of the engine (rule C12h: engine_semantic_encode / engine_semantic_head) against the CPU oracle's restatement (oracle/bark_oracle.cpp:
semantic_encode, hub_head), bit for bit: taps 0 - 5 and the ids at every frame count at which a kernel takes another path between 1 and 1024 frames (S1), on the
signals that reach the norm's corners (S2), behind a 1024-frame call whose scratch must not show (S3), on the cross-check routes (S4), the token head alone and on
exact ties (S5), and at HuBERT-base widths (S6).  tests/test_gpu_semantic_encoder.py pins the architecture to HuggingFace within a tolerance; this file pins the bits.
The oracle's encoder is pinned to the torch restatement and to HuggingFace without a GPU by tests/test_oracle_semantic_encoder.py, which also holds the condition
under which bit equality is decidable: on every input used here no erf GELU and no LSTM gate of the oracle's path lies within 8 double-ulps of the midpoint of two
floats (Oracle.near_midpoints() == 0; the seeds of semantic_encoder_ref.ORACLE_SEEDS were chosen for it), so the device's libm cannot round to another float than
the host's.  A difference here is a finding about a kernel."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import semantic_encoder_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300          # a child loads the toy model and the encoder and runs at most 20 calls of a few milliseconds each: seconds; nothing in it waits


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


def _hubert(preset):
    from tools.make_synth_hubert import ensure_hubert
    return ensure_hubert(preset, 0)


def _exact(name, got, want):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} vs {want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel())
        err = np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))
        first = np.unravel_index(bad[0], got.shape)
        raise AssertionError(f"{name}: {bad.size}/{got.size} elements differ, first at {tuple(int(i) for i in first)} "
                             f"(engine {got[first]!r}, oracle {want[first]!r}), max abs err {err:.3e}")


class _Env:
    """contexts and oracles per encoder file, made on first use and shared by the tests of the module"""

    def __init__(self, tmp):
        self.tmp, self.ctxs, self.orcs = tmp, {}, {}

    def ctx(self, hub_path, bark_preset="toy"):
        if hub_path not in self.ctxs:
            pkg = _pkg()
            c = pkg.BarkContext.load_model(_model(bark_preset), pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32), seed=0)
            c.load_semantic_encoder(hub_path)
            self.ctxs[hub_path] = c
        return self.ctxs[hub_path]

    def oracle(self, hub_path):
        """the oracle opens on the toy model whatever the engine's: the encoder file alone decides what the semantic encoder computes"""
        if hub_path not in self.orcs:
            from oracle.pyoracle import Oracle
            o = Oracle(_model("toy"), n_threads=8)
            o.load_semantic_encoder(hub_path)
            self.orcs[hub_path] = o
        return self.orcs[hub_path]

    def close(self):
        for c in self.ctxs.values():
            c.free()
        for o in self.orcs.values():
            o.close()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    e = _Env(str(tmp_path_factory.mktemp("semantic_encoder_oracle")))
    yield e
    e.close()


def _compare(name, ctx, orc, x, stages):
    want, want_ids = orc.semantic_encode_taps(x, stages)
    assert orc.near_midpoints() == 0, f"{name}: the input is not decidable bit for bit (tests/test_oracle_semantic_encoder.py holds the seeds)"
    for st in stages:
        _exact(f"{name} tap {st} ({ref.TAPS[st]})", ctx.semantic_encode_tap(x, st), want[st])
    _exact(f"{name} ids", ctx.semantic_encode(x), want_ids)


def _stages(n):
    return (1, 2, 3, 4, 5) if n >= ref.ORACLE_LONG else (0, 1, 2, 3, 4, 5)


# ---- S1 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.ORACLE_S1, ids=lambda v: f"n{v}_")
def test_frame_count_edges_equal_the_oracle(env, n):
    """hub_toy, taps 0 - 5 and the ids (from 327759 samples on taps 1 - 5: tap 0 is 65 550 x 128 values and more, and tap 1 depends on all of them).  T frames =
    (n - 400) // 320 + 1; each length is the smallest input that reaches its edge:
    400 / 719 / 720 (T 1, 1, 2): one row takes the one-row GEMV at K = 384; attention over one key and over two;
    2580 (T 7): 515 / 257 / 128 / 63 / 31 / 15 / 7 rows behind the seven convolutions (hub_stage_rows) - convolution 1 writes 257 rows, so the third 128-row
        workgroup of conv_down_mfma_kernel holds exactly one live row behind two full ones (5200: 1039 / 519 / 259 / 129 / 64 / 32 / 16, the same at convolution 3);
    2640 / 2960 (T 8, 9): Kp / 2 = 8 - every positional tap row is padding on one side;
    5129 / 5130 (T 15): T0 = 1024 and 1025 rows of convolution 0 - one and two chunks of the norm's partial sums;
    5200 / 5520 (T 16, 17): Kp = 16 frames;
    10000 / 10320 / 10640 (T 31, 32, 33): the 32-query attention tile, the 32-frame wave of the positional convolution;
    20240 / 20560 / 20880 (T 63, 64, 65): the 64-row GEMM tile, the LSTM's captured 64-step block;
    40720 / 41040 / 41360 (T 127, 128, 129): the 128-frame workgroup of the positional convolution, the second replay of the LSTM block;
    327759 (T 1023): the longest input on attn_rows_kernel, 65 chunks of the norm's partial sums, 16 replays of the LSTM block;
    327760 / 328079 (T 1024): attn_window_kernel<false> with HuBERT's six heads - the shortest and the longest input of 1024 frames."""
    path = _hubert("hub_toy")
    _compare(f"hub_toy n={n}", env.ctx(path), env.oracle(path), ref.oracle_signal(n), _stages(n))


# ---- S2 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.ORACLE_S2_SIGNALS)
def test_signals_at_the_norms_corners_equal_the_oracle(env, kind):
    """5200 samples (1039 rows of convolution 0: a wrong statistic is not averaged away).  zeros: the variance is exactly 0 in every channel, the norm's output
    is its bias; half (a constant 0.5): SS / T0 - mean^2 cancels to rounding noise of either sign - the clamp at 0; alternating (+1, -1): the largest
    convolution-0 outputs a recording can produce."""
    path = _hubert("hub_toy")
    _compare(f"hub_toy {kind} n={ref.ORACLE_S2_N}", env.ctx(path), env.oracle(path), ref.oracle_signal(ref.ORACLE_S2_N, kind), (0, 1, 2, 3, 4, 5))


# ---- S3 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_no_scratch_of_a_1024_frame_call_shows_in_later_calls(env):
    """One context, in order: 328079 samples of 0.9 x (+1, -1) - every scratch buffer filled to its last row with large values -, then the fixture signal at 400,
    10000, 10320, 10640 and 20880 samples.  Every call equals the oracle: a key, a frame of the positional convolution or an LSTM state left over from the long
    call is a bit difference here, not noise inside a tolerance."""
    path = _hubert("hub_toy")
    ctx, orc = env.ctx(path), env.oracle(path)
    for kind, n in ref.ORACLE_S3:
        _compare(f"hub_toy {kind} n={n} (in S3's order)", ctx, orc, ref.oracle_signal(n, kind), _stages(n))


# ---- S4 ---------------------------------------------------------------------------------------------------------------------------------------------
_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import semantic_encoder_ref as ref
from bark_amd_loader import load_package
pkg = load_package()
ctx = pkg.BarkContext.load_model(sys.argv[2], pkg.default_params(temp=0.0, fine_temp=0.0), 0)
ctx.load_semantic_encoder(sys.argv[3])
d = {}
for n in (int(v) for v in sys.argv[4].split(",")):
    x = ref.oracle_signal(n)
    for st in ((1, 2, 3, 4, 5) if n >= ref.ORACLE_LONG else range(6)):
        d["tap%%d_n%%d" %% (st, n)] = ctx.semantic_encode_tap(x, st)
    d["ids_n%%d" %% n] = ctx.semantic_encode(x)
np.savez(sys.argv[1], **d)
ctx.free()
''' % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("mask", ref.ORACLE_S4_MASKS, ids=lambda v: f"crosscheck{v}_")
def test_cross_check_routes_equal_the_oracle(env, mask):
    """One fresh process per mask (BARK_HIP_CROSSCHECK is read once per process) at 720, 10640 and 327760 samples.  512: attn_rows_kernel serves the 1024-frame
    input too; 1: gemv_rows_kernel forms every product; 1024: launch_conv_down sends the six strided convolutions to conv_down_chain_kernel (order C9) - the
    oracle follows with set_codec_mfma(False), as for the codec.  The other two masks leave every order as it is."""
    path = _hubert("hub_toy")
    orc = env.oracle(path)
    with tempfile.NamedTemporaryFile(suffix=".npz", delete=False, dir=env.tmp) as f:
        out = f.name
    r = subprocess.run([sys.executable, "-c", _CHILD, out, _model("toy"), path, ",".join(map(str, ref.ORACLE_S4_LENGTHS))],
                       env=dict(os.environ, BARK_HIP_CROSSCHECK=str(mask)), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stderr[-1500:]
    got = np.load(out)
    orc.set_codec_mfma(mask != 1024)
    try:
        for n in ref.ORACLE_S4_LENGTHS:
            want, want_ids = orc.semantic_encode_taps(ref.oracle_signal(n), _stages(n))
            assert orc.near_midpoints() == 0, (mask, n)
            for st in _stages(n):
                _exact(f"hub_toy n={n} tap {st} under BARK_HIP_CROSSCHECK={mask}", got[f"tap{st}_n{n}"], want[st])
            _exact(f"hub_toy n={n} ids under BARK_HIP_CROSSCHECK={mask}", got[f"ids_n{n}"], want_ids)
    finally:
        orc.set_codec_mfma(True)


# ---- S5 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ref.ORACLE_S5_T, ids=lambda v: f"T{v}_")
def test_head_alone_equals_the_oracle(env, T):
    """bark_hip_semantic_head on seeded random rows [T][H]: logits and ids.  1 and 2 rows: the one-row GEMV and the first step behind it; 63 / 64 / 65 and
    128 / 129: the captured 64-step LSTM block ends inside, at and behind a replay; 1024: sixteen replays and the largest row count the head takes."""
    path = _hubert("hub_toy")
    ctx, orc = env.ctx(path), env.oracle(path)
    feats = ref.head_rows(T, orc.semantic_hparams()["H"])
    want_ids, want_logits = orc.semantic_head(feats)
    assert orc.near_midpoints() == 0
    ids, logits = ctx.semantic_head(feats, want_logits=True)
    _exact(f"head T={T} logits", logits, want_logits)
    _exact(f"head T={T} ids", ids, want_ids)


def test_head_returns_the_lower_id_of_two_equal_classes(env):
    """A copy of the hub_toy file in which two pairs of rows of head.out.weight (and their bias entries) are equal - the pairs built on the two ids the reference
    head picks most often on these rows (ref.tie_pairs: a neighbour, and the class 64 below): every frame that picked one of them now sees two equal maxima.  The
    engine equals the oracle bit for bit, no frame answers the higher id of a pair, and both lower ids are answered."""
    hp, W = ref.load(_hubert("hub_toy"))
    feats = ref.head_rows(129, hp["H"])
    pairs = ref.tie_pairs(ref.head(hp, W, feats)[1], hp["n_classes"])
    path = os.path.join(env.tmp, "hubert_toy_ties.bin")
    ref.write_tie_hubert(_hubert("hub_toy"), path, pairs)
    ctx, orc = env.ctx(path), env.oracle(path)
    want_ids, want_logits = orc.semantic_head(feats)
    assert orc.near_midpoints() == 0
    ids, logits = ctx.semantic_head(feats, want_logits=True)
    _exact("tie file: logits", logits, want_logits)
    _exact("tie file: ids", ids, want_ids)
    for lo, hi, _ in pairs:
        assert np.array_equal(logits[:, lo], logits[:, hi])
        assert not (ids == hi).any(), (lo, hi, np.flatnonzero(ids == hi)[:4])
        assert (ids == lo).any(), (lo, hi)


# ---- S6 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.ORACLE_S6, ids=lambda v: f"hub_base-n{v}_")
def test_hubert_base_widths_equal_the_oracle(env, n):
    """hub_base (C 512, H 768, 12 heads, F 3072, 7 layers, Kp 128, G 16, D 1024, 10 000 classes) on the `small` model: hidden_states[0], the last layer, the
    logits and the ids.  16000 samples: 49 frames, fewer than the positional kernel is wide; 48000: 149 frames, the only case with Kp = 128 narrower than T, two
    workgroups of the positional convolution and three replays of the LSTM block at D = 1024.  The oracle recomputes both (0.3 s and 0.8 s on 8 threads)."""
    path = _hubert("hub_base")
    _compare(f"hub_base n={n}", env.ctx(path, "small"), env.oracle(path), ref.oracle_signal(n, preset="hub_base"), (3, 4, 5))
