"""The EnCodec decoder of the engine (engine_codec_decode_many: one utterance, and the batched form every lock-step job runs, reached here through
bark_hip_codec_decode_many) against the CPU oracle's decoder of each utterance alone (Oracle.codec_decode / codec_tap), bit for bit - no tolerance
anywhere in this file.  The oracle's decoder is pinned to numpy and HuggingFace without a GPU by tests/test_oracle_codec_decoder.py.

  D1  lengths, toy, one utterance, taps 0 - 5 and PCM: the 32-row matrix-core tile, the 128-row workgroup, the LSTM's captured 64-step block
  D2  ragged batches: utterance boundaries inside a wave tile, a 1-frame utterance between long ones, unequal lengths in the shared LSTM steps
  D3  toy / mini / EnCodec-24 kHz widths in both convolution orders and without graphs, one fresh process each
  D4  codebook depths n_q
  D5  one context through a sequence that replays, re-captures and drops the captured graphs; an encode between two decodes
  D6  refusals, after which the context still decodes
  D7  the longest input the door admits (4096 frames)

Codes are seeded default_rng draws; D1 - D5 each carry an utterance whose columns are all equal and one that uses only the ids 0 and 1023."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D1_LENGTHS = (1, 2, 6, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129)
RAGGED32 = tuple(1 + (7 * b) % 13 for b in range(32))
D2_LISTS = ((1, 1), (2, 1, 7), (33, 1, 31), (7, 65, 3), (64, 1), (1, 63, 2), (1, 33, 2, 65), (129, 1, 2), (3,) * 32, RAGGED32)
D3_LISTS = ((1,), (2,), (33,), (1, 33, 2, 65), RAGGED32)
D3_TAP_LENGTHS = (1, 2, 33)
A = (7, 65)


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


def draw(seed, n_q, T):
    return np.random.default_rng(seed).integers(0, 1024, (n_q, T)).astype(np.int32)


def equal_columns(seed, n_q, T):
    """every frame carries the same column of ids"""
    return np.repeat(draw(seed, n_q, 1), T, axis=1).copy()


def extremes(seed, n_q, T):
    """only the first and the last row of every codebook"""
    return (1023 * np.random.default_rng(seed).integers(0, 2, (n_q, T))).astype(np.int32)


def codes_of_list(Ts, n_q=8, seed=0):
    """one matrix per utterance, different content in each"""
    return [draw(100000 * seed + 1000 * b + T, n_q, T) for b, T in enumerate(Ts)]


def special_pair(n_q=8, seed=0):
    """the two extra utterances of a family: 33 frames of one column, 7 frames of ids 0 / 1023"""
    return [equal_columns(7000 + seed, n_q, 33), extremes(7100 + seed, n_q, 7)]


def _exact(name, got, want, per_frame=None):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} vs {want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel())
        err = np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))
        where = f", frame {bad[0] // per_frame}" if per_frame else ""
        raise AssertionError(f"{name}: {bad.size}/{got.size} elements differ, first at {bad[0]}{where} "
                             f"(engine {got.ravel()[bad[0]]!r}, oracle {want.ravel()[bad[0]]!r}), max abs err {err:.3e}")


class _Env:
    """contexts and oracles per preset, made on first use and shared by the tests of the module; the oracle's results are computed once per input"""

    def __init__(self, tmp):
        self.tmp, self.ctxs, self.orcs, self.done = tmp, {}, {}, {}

    def new_ctx(self, preset):
        pkg = _pkg()
        return pkg.BarkContext.load_model(_model(preset), pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32), seed=0)

    def ctx(self, preset):
        if preset not in self.ctxs:
            self.ctxs[preset] = self.new_ctx(preset)
        return self.ctxs[preset]

    def oracle(self, preset):
        if preset not in self.orcs:
            from oracle.pyoracle import Oracle
            self.orcs[preset] = Oracle(_model(preset), n_threads=8)
        return self.orcs[preset]

    def want(self, preset, codes, stage=-1, mfma=True):
        """the oracle's PCM (stage -1) or tap of one utterance alone"""
        key = (preset, stage, mfma, codes.shape, codes.tobytes())
        if key not in self.done:
            orc = self.oracle(preset)
            orc.set_codec_mfma(mfma)
            try:
                r = orc.codec_decode(codes) if stage < 0 else orc.codec_tap(codes, stage)
            finally:
                orc.set_codec_mfma(True)
            r.setflags(write=False)
            self.done[key] = r
        return self.done[key]

    def close(self):
        for c in self.ctxs.values():
            c.free()
        for o in self.orcs.values():
            o.close()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    e = _Env(str(tmp_path_factory.mktemp("codec_decoder")))
    yield e
    e.close()


def _batch_against_oracle_and_singles(env, ctx, preset, cl, name, singles=True):
    """one codec_decode_many: every utterance equals the oracle's decode of it alone and - the same statement about the engine - its own single call"""
    many = ctx.codec_decode_many(cl)
    assert len(many) == len(cl)
    for b, (codes, got) in enumerate(zip(cl, many)):
        what = f"{name}: utterance {b} ({codes.shape[1]} frames, n_q {codes.shape[0]}) of {len(cl)}"
        _exact(what + " against the oracle", got, env.want(preset, codes), 320)
        if singles:
            _exact(what + " against the single call", got, ctx.codec_decode(codes), 320)
    return many


# ---- D1 ---------------------------------------------------------------------------------------------------------------------------------------------
def _taps_and_pcm(env, ctx, preset, codes, name):
    T = codes.shape[1]
    rows = 1
    for st in range(6):
        if st >= 2:
            rows *= (8, 5, 4, 2)[st - 2]
        got = ctx.codec_tap(codes, st)
        want = env.want(preset, codes, st)
        assert got.size % (T * rows) == 0
        # [C][T rows]: report the first differing element as (channel, row)
        _exact(f"{name} tap {st}", got.reshape(-1, T * rows), want.reshape(-1, T * rows))
    _exact(f"{name} PCM", ctx.codec_decode(codes), env.want(preset, codes), 320)


@pytest.mark.parametrize("T", D1_LENGTHS, ids=lambda v: f"T{v}_")
def test_lengths_taps_and_pcm_equal_the_oracle(env, T):
    """D1.  31 / 32 / 33: one 32-row matrix-core tile, then a second tile with one live lane; 127 / 128 / 129: the 128-row workgroup; 63 / 64 / 65: the
    LSTM's captured 64-step block (Tmax = 63 replays once; 64 twice, the second block running only layer 2's last step); 1, 2, 6: the padding rule's
    short-input detours, 7 the first length without one."""
    _taps_and_pcm(env, env.ctx("toy"), "toy", draw(T, 8, T), f"toy T={T}")


@pytest.mark.parametrize("kind", ["equal_columns", "ids_0_and_1023"])
def test_special_codes_taps_and_pcm_equal_the_oracle(env, kind):
    codes = special_pair()[0 if kind == "equal_columns" else 1]
    _taps_and_pcm(env, env.ctx("toy"), "toy", codes, f"toy {kind} T={codes.shape[1]}")


# ---- D2 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(D2_LISTS)), ids=lambda k: f"list{k}_" + ("x".join(map(str, D2_LISTS[k])) if len(D2_LISTS[k]) < 8 else f"{len(D2_LISTS[k])}utt"))
def test_ragged_batches_equal_the_oracle_and_the_single_call(env, k):
    """D2.  Prefix sums that 4 does not divide put an utterance boundary inside a 32-row wave tile at the upsampling factors 1, 8 and 40 (at 160 and 320
    the boundaries are tile-aligned by arithmetic and only the workgroup straddles them); a 1-frame utterance between long ones shows a transposed
    convolution or a reflected pad that reads its neighbour's rows; unequal lengths show LSTM steps taken for utterances that have ended."""
    Ts = D2_LISTS[k]
    _batch_against_oracle_and_singles(env, env.ctx("toy"), "toy", codes_of_list(Ts, seed=k + 1), f"toy {list(Ts)}")


def test_ragged_batch_with_special_codes(env):
    """[2, 33 equal columns, 1, 7 of ids 0 / 1023]"""
    eq, ex = special_pair(seed=2)
    _batch_against_oracle_and_singles(env, env.ctx("toy"), "toy", [draw(21, 8, 2), eq, draw(22, 8, 1), ex], "toy special batch")


# ---- D3 ---------------------------------------------------------------------------------------------------------------------------------------------
def _d3_inputs():
    """{name: [matrices]} of a child's batches, {name: matrix} of its tapped utterances"""
    lists = {"list%d" % k: codes_of_list(Ts, seed=40 + k) for k, Ts in enumerate(D3_LISTS)}
    lists["special"] = special_pair(seed=3)
    taps = {"T%d" % T: draw(300 + T, 8, T) for T in D3_TAP_LENGTHS}
    return lists, taps


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_codec_decoder as t
pkg = t._pkg()
ctx = pkg.BarkContext.load_model(sys.argv[2], pkg.default_params(temp=0.0, fine_temp=0.0), 0)
lists, taps = t._d3_inputs()
d = {}
for name, cl in lists.items():
    for b, pcm in enumerate(ctx.codec_decode_many(cl)):
        d["%%s_u%%d" %% (name, b)] = pcm
for name, codes in taps.items():
    for st in range(6):
        d["%%s_tap%%d" %% (name, st)] = ctx.codec_tap(codes, st)
np.savez(sys.argv[1], **d)
ctx.free()
''' % (ROOT, os.path.join(ROOT, "tests"))

D3_MODES = {"c9m": (dict(BARK_HIP_CROSSCHECK="0"), True), "c9": (dict(BARK_HIP_CROSSCHECK="1024"), False),
            "c9m_no_graphs": (dict(BARK_HIP_CROSSCHECK="0", BARK_HIP_GRAPH="0"), True)}


@pytest.mark.parametrize("mode", list(D3_MODES))
@pytest.mark.parametrize("preset", ["toy", "mini", "small"])
def test_widths_and_orders_equal_the_oracle(env, preset, mode):
    """D3.  One fresh process per (preset, order) - the mask BARK_HIP_CROSSCHECK and BARK_HIP_GRAPH are read once per process: C9m (the matrix cores; at
    mini and small every convolution is C9m), C9 (bit 1024: the chain kernels everywhere, the oracle follows with set_codec_mfma(False)), and C9m with
    graphs off.  Batches [1], [2], [33], [1, 33, 2, 65], the ragged 32 and the special pair; taps 0 - 5 at 1, 2 and 33 frames."""
    extra, mfma = D3_MODES[mode]
    with tempfile.NamedTemporaryFile(suffix=".npz", delete=False, dir=env.tmp) as f:
        out = f.name
    r = subprocess.run([sys.executable, "-c", _CHILD, out, _model(preset)], env=dict(os.environ, **extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    got = np.load(out)
    lists, taps = _d3_inputs()
    for name, codes in taps.items():
        for st in range(6):
            _exact(f"{preset} {mode} {name} tap {st}", got[f"{name}_tap{st}"], env.want(preset, codes, st, mfma))
    for name, cl in lists.items():
        for b, codes in enumerate(cl):
            _exact(f"{preset} {mode} {name}: utterance {b} ({codes.shape[1]} frames) of {len(cl)}", got[f"{name}_u{b}"], env.want(preset, codes, -1, mfma), 320)
    os.unlink(out)


# ---- D4 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n_q", [("toy", 1), ("toy", 2), ("toy", 8), ("small", 2), ("small", 8), ("small", 32)], ids=lambda v: str(v))
def test_codebook_depths_equal_the_oracle(env, preset, n_q):
    """D4: [5, 1, 33] and the special pair at every depth; rvq_gather_kernel reads utterance b's matrix at n_q Tpre[b] with row pitch T[b]."""
    ctx = env.ctx(preset)
    _batch_against_oracle_and_singles(env, ctx, preset, codes_of_list((5, 1, 33), n_q, seed=60 + n_q), f"{preset} n_q={n_q} [5, 1, 33]")
    _batch_against_oracle_and_singles(env, ctx, preset, special_pair(n_q, seed=4), f"{preset} n_q={n_q} special pair")


# ---- D5 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regrow", [True, False], ids=["with_regrow", "without_regrow"])
def test_one_context_through_replays_recaptures_and_regrowth(env, regrow):
    """D5, a context of its own, in this order: A = [7, 65]; A again (the tail graph replays); A with new codes; [65, 7] (same counts, other order: the
    tail graph is keyed by the list); [9, 2] (same B, other T: the LSTM capture is kept, the tail is re-captured); one utterance of 3; one of 200
    (`with_regrow`: the buffers grow, both captures must be dropped); [1, 1]; the special pair; A with the first codes, which must give the bits of
    step 1.  Every result against the oracle."""
    ctx = env.new_ctx("toy")
    try:
        first = codes_of_list(A, seed=70)
        step1 = _batch_against_oracle_and_singles(env, ctx, "toy", first, "step 1, A", singles=False)
        again = _batch_against_oracle_and_singles(env, ctx, "toy", first, "step 2, A again", singles=False)
        for x, y in zip(step1, again):
            assert np.array_equal(x, y)
        _batch_against_oracle_and_singles(env, ctx, "toy", codes_of_list(A, seed=71), "step 3, A with new codes", singles=False)
        _batch_against_oracle_and_singles(env, ctx, "toy", codes_of_list((65, 7), seed=72), "step 4, [65, 7]", singles=False)
        _batch_against_oracle_and_singles(env, ctx, "toy", codes_of_list((9, 2), seed=73), "step 5, [9, 2]", singles=False)
        single = draw(74, 8, 3)
        _exact("step 6, [3] single", ctx.codec_decode(single), env.want("toy", single), 320)
        if regrow:
            _batch_against_oracle_and_singles(env, ctx, "toy", codes_of_list((200,), seed=75), "step 7, [200]", singles=False)
        _batch_against_oracle_and_singles(env, ctx, "toy", codes_of_list((1, 1), seed=76), "step 8, [1, 1]", singles=False)
        _batch_against_oracle_and_singles(env, ctx, "toy", special_pair(seed=5), "the special pair", singles=False)
        last = _batch_against_oracle_and_singles(env, ctx, "toy", first, "step 9, A with the first codes", singles=False)
        for b, (x, y) in enumerate(zip(step1, last)):
            _exact(f"step 9 against step 1, utterance {b}", y, x, 320)
    finally:
        ctx.free()


def test_an_encode_between_two_decodes(env):
    """toy_enc: the scratch buffers and the LSTM's rows are shared by both directions (the captured blocks are not): the two decodes of A are equal and
    the oracle's, the encode in between equals the oracle's."""
    import codec_encoder_ref
    ctx, orc = env.ctx("toy_enc"), env.oracle("toy_enc")
    first = codes_of_list(A, seed=77)
    one = _batch_against_oracle_and_singles(env, ctx, "toy_enc", first, "A before the encode", singles=False)
    x = codec_encoder_ref.fixture_signal(977)
    _exact("codes of the encode between", ctx.codec_encode(x, 8), orc.codec_encode(x, 8))
    two = _batch_against_oracle_and_singles(env, ctx, "toy_enc", first, "A after the encode", singles=False)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


# ---- D6 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_decoding(env):
    """D6: a T of 0 and of 4097, a code of -1 and of 1024, n_q of 0 and of one above the file's 8, 33 utterances: each returns -1, each in either place
    of a pair where it has one, and after every one of them the same context decodes A to the oracle's bits."""
    ctx = env.ctx("toy")
    lib, h = ctx._lib, ctx._h
    first = codes_of_list(A, seed=78)
    pcm = np.zeros(320 * (4097 + 65 + 33 * 3), np.float32)         # never the reason of a refusal below

    def many(cl, T=None, n_q=8, n=None):
        ptrs = (C.c_void_p * len(cl))(*[c.ctypes.data for c in cl])
        Ts = np.asarray([c.shape[1] for c in cl] if T is None else T, np.int32)
        return lib.bark_hip_codec_decode_many(h, ptrs, Ts.ctypes.data, len(cl) if n is None else n, n_q, pcm.ctypes.data, pcm.size)

    def still_decodes(after):
        _batch_against_oracle_and_singles(env, ctx, "toy", first, f"A after {after}", singles=False)

    assert many(first) == 320 * sum(A)
    long = np.zeros((8, 4097), np.int32)
    for where in (0, 1):
        pair = list(first)
        assert many(pair, T=[0, 65] if where == 0 else [7, 0]) == -1
        still_decodes(f"T = 0 in place {where}")
        pair[where] = long
        assert many(pair) == -1
        still_decodes(f"T = 4097 in place {where}")
        for bad in (-1, 1024):
            for spot in ((0, 0), (7, -1)):                        # the first id of the matrix and its last
                pair = [c.copy() for c in first]
                pair[where][spot] = bad
                assert many(pair) == -1, (where, bad, spot)
                still_decodes(f"a code of {bad} in place {where}")
    assert lib.bark_hip_codec_decode(h, long.ctypes.data, 8, 4097, pcm.ctypes.data, pcm.size) == -1
    assert lib.bark_hip_codec_decode(h, long.ctypes.data, 8, 0, pcm.ctypes.data, pcm.size) == -1
    for n_q in (0, 9, -1):
        assert many(first, n_q=n_q) == -1
        still_decodes(f"n_q = {n_q}")
    crowd = [draw(900 + b, 8, 3) for b in range(33)]
    assert many(crowd) == -1
    still_decodes("33 utterances")
    assert many(crowd[:32]) == 320 * 96
    assert lib.bark_hip_codec_decode_many(h, (C.c_void_p * 2)(*[c.ctypes.data for c in first]), np.asarray(A, np.int32).ctypes.data, 2, 8,
                                          pcm.ctypes.data, 320 * sum(A) - 1) == -1
    still_decodes("a short capacity")


# ---- D7 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_longest_admitted_input_equals_the_oracle(env):
    """D7: one utterance of 4096 frames, the largest the door admits (1 310 720 samples, 65 replays of the LSTM block), PCM only."""
    codes = draw(4096, 8, 4096)
    _exact("toy T=4096 PCM", env.ctx("toy").codec_decode(codes), env.want("toy", codes), 320)
