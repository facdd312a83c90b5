"""GPU tests of loudness levelling (rule C17l): the two kernels bit for bit against tests/loudness_ref.py fed with the library's own
constants and target mean squares - the z table, the block counts, the gain as f32 bits and the levelled samples; lufs within 1e-9 - at the smallest lengths
where something changes, on silence, under the absolute gate, on a composite that the relative gate splits, with the ceiling and the cap binding, as a ragged
batch of 64 against single calls; then the routes (level_many in front of tempo, rate and format; audio_with, batch_audio_with, long_audio_with on the toy
model; the request collector; bark_batch_server's "loudness" field) byte for byte, and the refusals."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import loudness_ref as lr
import output_format_ref as ofr
import tempo_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "hello world this is bark"
LONG_TEXT = "hello world. this is bark"
TARGET = -16.0
EDGE_LENGTHS = [2399, 9599, 9600, 9601, 11999, 12000, 12001, 16800]              # under a hop, under a block, one block, two blocks, the first full warm-up
WAVE_LENGTHS = [63 * 2400, 63 * 2400 + 1, 64 * 2400, 64 * 2400 + 1, 65 * 2400, 65 * 2400 + 1]      # 63, 64, 65 hops: around one wave of lanes
KINDS = ["silence", "under_gate", "composite", "spike", "quiet"]


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


def _load(preset="toy", **over):
    pkg = _pkg()
    par = dict(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32)
    par.update(over)
    return pkg.BarkContext.load_model(_model(preset), pkg.default_params(**par), seed=0)


@pytest.fixture(scope="module")
def ctx():
    c = _load()
    yield c
    c.free()


@pytest.fixture(scope="module")
def consts():
    """the library's own constants and its target mean square for TARGET"""
    lib = _pkg().load_library()
    k = np.zeros(9, np.float64)
    assert lib.bark_hip_loudness_constants(k.ctypes.data_as(C.POINTER(C.c_double))) == 9
    return k, lib.bark_hip_loudness_target_ms(int(round(100 * TARGET)))


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}.get(got.dtype.itemsize) if got.dtype.kind == "f" else None
    bad = np.flatnonzero(got.view(bits) != want.view(bits)) if bits else np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:5]]} != {want.reshape(-1)[bad[:5]]}"


def noise(n: int, amp: float, seed) -> np.ndarray:
    return np.random.default_rng([17, *np.atleast_1d(seed)]).uniform(-amp, amp, n).astype(np.float32)


def signal(kind, n=None) -> np.ndarray:
    if kind == "noise":
        return noise(n, 0.1, n)
    if kind == "silence":
        return np.zeros(12000, np.float32)
    if kind == "under_gate":                                                # -85 LUFS: every block fails the absolute gate
        return noise(14400, 1e-4, 1)
    if kind == "composite":                                                 # loud, 40 dB quieter (over the absolute gate, under the relative one), silent
        return np.concatenate([noise(24000, 0.3, 2), noise(24000, 0.003, 3), np.zeros(24000, np.float32)])
    if kind == "spike":                                                     # the ceiling binds: 1 / 0.9 is less than the gain to the target and than the cap
        x = noise(12000, 0.01, 4); x[7000] = -0.9
        return x
    assert kind == "quiet"                                                  # the cap binds: about -65 LUFS, 49 dB under the target, a peak of 0.001
    return noise(12000, 0.001, 5)


CASES = [("noise", n) for n in EDGE_LENGTHS + WAVE_LENGTHS] + [(k, None) for k in KINDS]
_REF = {}


def references(consts):
    """{case: (y, info)} of the rule for every case, the hop runs of all of them in one pass, shared by the tests"""
    if not _REF:
        k, tms = consts
        for case, r in zip(CASES, lr.level_many([signal(*c) for c in CASES], tms, 1.0, 10.0, k=k)):
            _REF[case] = r
    return _REF


def _check(what, x, got_y, got_info, got_z, want):
    y, info = want
    _same(f"{what}: z", got_z, info["z"])
    assert (got_info["n_blocks"], got_info["n_abs"], got_info["n_gated"]) == (info["n_blocks"], info["n_abs"], info["n_gated"]), (what, got_info, info)
    _same(f"{what}: gain", np.float32(got_info["gain"]), info["gain"])
    _same(f"{what}: samples", got_y, y)
    assert got_info["flags"] == info["flags"], (what, got_info["flags"], info["flags"])
    _same(f"{what}: peak", np.float32(got_info["peak"]), info["peak"])
    _same(f"{what}: mean square", np.float64(got_info["mean_square"]), np.float64(info["mean_square"]))
    if info["flags"] & lr.UNMEASURABLE:
        assert got_info["gain"] == 1.0 and got_y.tobytes() == x.tobytes() and got_info["lufs"] == -math.inf
    else:
        assert abs(got_info["lufs"] - info["lufs"]) <= 1e-9, (what, got_info["lufs"], info["lufs"])


# ---- T1: the kernels against the rule ---------------------------------------------------------------------------------------------------------------------
def test_the_reference_cases_are_what_they_claim(consts):
    """asserted on the restatement alone, so that no case degenerates silently"""
    ref = references(consts)
    for n in (2399, 9599):
        info = ref[("noise", n)][1]
        assert info["flags"] == lr.UNMEASURABLE and info["gain"] == 1.0 and info["n_blocks"] == 0
    assert [ref[("noise", n)][1]["n_blocks"] for n in (9600, 9601, 11999, 12000, 12001, 16800)] == [1, 1, 1, 2, 2, 4]
    assert [ref[("noise", n)][1]["n_blocks"] for n in WAVE_LENGTHS] == [60, 60, 61, 61, 62, 62]
    for n in EDGE_LENGTHS[2:] + WAVE_LENGTHS:
        info = ref[("noise", n)][1]
        assert info["flags"] == 0 and info["n_gated"] == info["n_blocks"] and 1.0 < info["gain"] < 10.0, (n, info)
    s = ref[("silence", None)][1]
    assert s["flags"] == lr.UNMEASURABLE and s["n_blocks"] == 2 and s["n_abs"] == 0 and not s["z"].any()
    u = ref[("under_gate", None)][1]
    assert u["flags"] == lr.UNMEASURABLE and u["n_blocks"] == 3 and u["n_abs"] == 0 and u["z"].all() and u["gain"] == 1.0
    c = ref[("composite", None)][1]
    assert 0 < c["n_gated"] < c["n_abs"] < c["n_blocks"], c
    p = ref[("spike", None)][1]
    assert p["flags"] == lr.CEILING_BOUND and p["gain"] == np.float32(np.float64(1.0) / np.float64(np.float32(0.9)))
    q = ref[("quiet", None)][1]
    assert q["flags"] == lr.CAP_BOUND and q["gain"] == 10.0 and q["n_gated"] > 0


@pytest.mark.parametrize("case", CASES, ids=[f"{k}{'' if n is None else n}" for k, n in CASES])
def test_kernels_are_c17l_bit_for_bit(ctx, consts, case):
    x = signal(*case)
    ys, infos = ctx.level_many([x], TARGET, want_info=True)
    _check(str(case), x, ys[0], infos[0], ctx.loudness_hops(x), references(consts)[case])
    m = ctx.loudness(x)                                                                        # measure only: the same record, gain 1
    assert m["gain"] == 1.0 and {k: v for k, v in m.items() if k not in ("gain", "flags")} == {k: v for k, v in infos[0].items() if k not in ("gain", "flags")}
    assert ctx.loudness(x, TARGET) == infos[0]                                                 # .. and with the target: the gain it would apply


# ---- T2: a ragged batch of 64 -----------------------------------------------------------------------------------------------------------------------------
def test_a_ragged_batch_of_64_equals_64_single_calls(ctx, consts):
    ref = references(consts)
    order = [CASES[i % len(CASES)] for i in range(64)]
    xs = [signal(*c) for c in order]
    targets = [None if i % 7 == 3 else TARGET for i in range(64)]                            # some ride along unlevelled
    ys, infos = ctx.level_many(xs, targets, want_info=True)
    measured = ctx.loudness_many(xs, TARGET)
    for i, (case, x, t) in enumerate(zip(order, xs, targets)):
        want_y, want = ref[case]
        if t is None:
            assert ys[i].tobytes() == x.tobytes() and infos[i]["gain"] == 1.0 and infos[i]["n_gated"] == want["n_gated"]
        else:
            _check(f"segment {i} {case}", x, ys[i], infos[i], want["z"], (want_y, want))
            one_y, one = ctx.level_many([x], TARGET, want_info=True)
            assert one[0] == infos[i] and one_y[0].tobytes() == ys[i].tobytes(), (i, case)
        assert measured[i]["gain"] == want["gain"] and measured[i]["mean_square"] == want["mean_square"], (i, case)


# ---- T3: level_many in front of tempo, rate and format ---------------------------------------------------------------------------------------------------
def test_level_many_feeds_tempo_rate_and_format_on_the_device(ctx, consts):
    lib = ctx._lib
    case = ("noise", 12001)
    x = signal(*case)
    y = references(consts)[case][0]
    w = np.zeros(tr.W, np.float32)
    assert lib.bark_hip_tempo_window(w.ctypes.data) == tr.W
    lmh = np.zeros(3, np.int32)
    n = lib.bark_hip_resample_table(24000, 16000, None, 0, lmh.ctypes.data)
    h = np.zeros(n, np.float32)
    assert lib.bark_hip_resample_table(24000, 16000, h.ctypes.data, n, lmh.ctypes.data) == n
    h = h.reshape(int(lmh[0]), 2 * int(lmh[2]))
    fast = tr.tempo(y, 1250, w)
    got = ctx.level_many([x, x], [TARGET, None], [1.25, 1.0])
    _same("levelled, 1.25, 24000 f32", got[0], fast)
    assert got[1].tobytes() == x.tobytes()
    got = ctx.level_many([x, x], TARGET, [1.25, 1.0], 16000, "s16")
    _same("levelled, 1.25, 16000 s16", got[0], ofr.to_format(ofr.resample(fast, 24000, 16000, h=h), ofr.S16))
    _same("levelled, 1.0, 16000 s16", got[1], ofr.to_format(ofr.resample(y, 24000, 16000, h=h), ofr.S16))
    _same("levelled, 1.0, 24000 mu-law", ctx.level_many([x], TARGET, None, 24000, "mulaw")[0], ofr.to_format(y, ofr.MULAW))
    assert ctx.level_many([x], None, [1.25])[0].tobytes() == ctx.tempo(x, 1.25).tobytes()      # every request off: the tempo call itself


# ---- T4: the routes on the toy model ------------------------------------------------------------------------------------------------------------------------
def _level_ref(pcm, consts, target=TARGET):
    k, _ = consts
    return lr.level(pcm, _pkg().load_library().bark_hip_loudness_target_ms(int(round(100 * target))), 1.0, 10.0, k=k)


def test_audio_with_and_batch_audio_with_are_the_rule_over_the_result(ctx, consts):
    pkg = _pkg()
    assert ctx.generate_audio(TEXT)
    pcm = np.asarray(ctx.audio_data(), np.float32).copy()
    want, info = _level_ref(pcm, consts)
    got, ginfo = ctx.audio_with(loudness=TARGET, want_info=True)
    print("toy result:", len(pcm), "samples,", info["n_blocks"], "blocks, gain", info["gain"], "flags", info["flags"])
    _same("audio_with", got, want)
    _same("audio_with gain", np.float32(ginfo["gain"]), info["gain"])
    assert (ginfo["n_blocks"], ginfo["n_abs"], ginfo["n_gated"], ginfo["flags"]) == (info["n_blocks"], info["n_abs"], info["n_gated"], info["flags"])
    _same("audio_with 1.25 at 16000 s16", ctx.audio_with(16000, "s16", 1.25, TARGET), ctx.tempo_many([want], [1.25], 16000, "s16")[0])
    for rate, name, speed in ((24000, "f32", 1.0), (48000, "s16", 1.0), (8000, "mulaw", 1.25)):      # loudness off: the bytes of the _at form
        got, ginfo = ctx.audio_with(rate, name, speed, None, want_info=True)
        assert got.tobytes() == ctx.audio_at(speed, rate, name).tobytes() and ginfo["gain"] == 1.0 and ginfo["n_blocks"] == 0
    assert np.asarray(ctx.audio_data(), np.float32).tobytes() == pcm.tobytes()
    how = pkg.audio_render(16000, "s16", 1.25, TARGET)
    nb = 2 * ofr.n_out(tr.out_len(len(pcm), 1250), 24000, 16000)
    buf = np.zeros(nb, np.uint8)
    assert ctx._lib.bark_hip_get_audio_with(ctx._h, C.byref(how), buf.ctypes.data, nb - 1, None) == -2 - nb          # too small: -(2 + bytes)
    assert ctx._lib.bark_hip_get_audio_with(ctx._h, C.byref(how), buf.ctypes.data, nb, None) == nb
    for bad in (pkg.audio_render(16000, "s16", 1.25, -3.0), pkg.audio_render(16000, "s16", 1.25, -41.0), pkg.audio_render(16000, "s16", 2.5, TARGET),
                pkg.audio_render(11025, "s16", 1.0, TARGET), pkg.audio_render(loudness=TARGET, peak_ceiling=-1.0), pkg.audio_render(loudness=TARGET, max_gain=math.inf),
                pkg.audio_render(loudness=TARGET, peak_ceiling=math.nan)):
        assert ctx._lib.bark_hip_get_audio_with(ctx._h, C.byref(bad), buf.ctypes.data, nb, None) == -1
    res = ctx.generate_batch([TEXT, "another one"])
    assert all(r is not None for r in res)
    for i, r in enumerate(res):
        want, info = _level_ref(r["pcm"], consts, -23.0)
        got, ginfo = ctx.batch_audio_with(i, loudness=-23.0, want_info=True)
        _same(f"batch_audio_with {i}", got, want)
        _same(f"batch_audio_with {i} gain", np.float32(ginfo["gain"]), info["gain"])
        assert ctx.batch_audio_with(i, 48000, "s16", 0.8).tobytes() == ctx.batch_audio_at(i, 0.8, 48000, "s16").tobytes()
    assert ctx._lib.bark_hip_batch_audio_with(ctx._h, 2, C.byref(how), buf.ctypes.data, nb, None) == -1


@pytest.mark.lock_step_job
def test_long_audio_with_levels_every_chunk_on_its_own(ctx, consts):
    pkg = _pkg()
    join = pkg.join_params(gap_samples=600, fade_samples=48, trim_threshold=0.02)
    chunks = ctx.generate_long(LONG_TEXT, join=join, params=ctx.request_params(seed=5))
    assert len(chunks) == 2
    refs = [_level_ref(c["pcm"], consts) for c in chunks]
    levelled = [r[0] for r in refs]
    for rate, name in ((24000, "f32"), (16000, "s16")):
        got, infos = ctx.long_audio_with(rate, name, 1.0, TARGET, want_info=True)
        _same(f"long_audio_with {rate} {name}", got, ctx.join_many(levelled, join, rate, name))
        assert len(infos) == 2
        for gi, (_, info) in zip(infos, refs):
            _same("a chunk's gain", np.float32(gi["gain"]), info["gain"])
            assert gi["n_gated"] == info["n_gated"]
        assert ctx.long_audio_with(rate, name, 1.25).tobytes() == ctx.long_audio_at(1.25, rate, name).tobytes()
        assert ctx.long_audio_with(rate, name).tobytes() == ctx.long_audio_as(rate, name).tobytes()
        _same(f"long_audio_with {rate} {name} once more", ctx.long_audio_with(rate, name, 1.0, TARGET), ctx.join_many(levelled, join, rate, name))
    _same("another target is another join", ctx.long_audio_with(loudness=-23.0), ctx.join_many([_level_ref(c["pcm"], consts, -23.0)[0] for c in chunks], join))
    fast = ctx.tempo_many(levelled, [1.25, 1.25])
    _same("long_audio_with at 1.25", ctx.long_audio_with(speed=1.25, loudness=TARGET), ctx.join_many(fast, join))
    bad = pkg.audio_render(loudness=-3.0)
    assert ctx._lib.bark_hip_long_audio_with(ctx._h, C.byref(bad), None, 0, None, 0) == -1
    info1 = (pkg.BarkHipLoudnessInfo * 1)()
    assert ctx._lib.bark_hip_long_audio_with(ctx._h, C.byref(pkg.audio_render(loudness=TARGET)), None, 0, info1, 1) == -1      # two chunks, room for one record


@pytest.mark.concurrency
def test_collector_serves_a_job_in_which_only_some_requests_level(ctx, consts):
    pkg = _pkg()
    texts = [TEXT, "another one", "third", "and a fourth"]
    louds = [TARGET, None, -23.0, None]
    speeds = [None, None, 1.25, 0.8]
    fmts = [None, None, pkg.audio_format(8000, "mulaw"), pkg.audio_format(48000, "s16")]
    join = pkg.join_params(gap_samples=600)
    owner = _load(temp=0.7, fine_temp=0.5)
    try:
        with pkg.Batcher(owner, max_batch=8, max_wait_ms=200) as b:
            tickets = [b.submit(t, seed=40 + i, audio_format=f, speed=s, loudness=l) for i, (t, s, f, l) in enumerate(zip(texts, speeds, fmts, louds))]
            plain = [b.submit(t, seed=40 + i) for i, t in enumerate(texts)]                  # the same requests in the engine's own form
            long_level = b.submit(LONG_TEXT, seed=60, long=pkg.BarkHipLongParams(0, 0, join), loudness=TARGET)
            got = [b.wait_bytes(t) for t in tickets]
            ref = [b.wait(t) for t in plain]
            got_long = b.wait_bytes(long_level)
            assert b._lib.bark_hip_batcher_submit_with(b._b, b"x", None, None, None, C.byref(pkg.audio_render(loudness=-3.0))) == -1
            assert b._lib.bark_hip_batcher_submit_with(b._b, b"x", None, None, None, None) == -1
            assert b._lib.bark_hip_batcher_submit_long_with(b._b, b"x. y", None, None, None, None, C.byref(pkg.audio_render(loudness=TARGET, max_gain=-1.0))) == -1
        owner.generate_long(LONG_TEXT, join=join, params=owner.request_params(seed=60))
        want_long = owner.long_audio_with(loudness=TARGET)
    finally:
        owner.free()
    _same("request 0 levelled", got[0], _level_ref(ref[0], consts)[0])
    assert got[1].dtype == np.float32 and got[1].tobytes() == ref[1].tobytes()
    _same("request 2 at -23, 1.25, 8000 mu-law", got[2], ctx.tempo_many([_level_ref(ref[2], consts, -23.0)[0]], [1.25], 8000, "mulaw")[0])
    _same("request 3 at 0.8 in 48000 s16, not levelled", got[3], ctx.tempo_many([ref[3]], [0.8], 48000, "s16")[0])
    _same("the long text levelled", got_long, want_long)
    assert len(got_long) > 0


# ---- T5: the server -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.concurrency
def test_native_batch_server_loudness_field():
    from test_gpu_output_format import _chunks
    from test_gpu_voice_from_audio import _Server
    model = _model("toy")
    with _Server("-m", model) as srv:
        st, level = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7, "loudness": -16}).encode())
        assert st == 200
        st, level_mu = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7, "loudness": -16, "speed": 1.25, "sample_rate": 8000, "format": "mulaw"}).encode())
        assert st == 200
        st, long_level = srv.request("POST", "/bark", json.dumps({"text": LONG_TEXT, "seed": 7, "loudness": -23.5, "long": True, "gap_ms": 25}).encode())
        assert st == 200
        for bad in (-3, "x", -40.5, 0, True):
            assert srv.request("POST", "/bark", json.dumps({"text": TEXT, "loudness": bad}).encode())[0] == 400, bad
    with _Server("-m", model, "--loudness", "-16") as srv:
        st, level2 = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7}).encode())
        assert st == 200 and level2 == level
    one = _load(n_steps_text_encoder=768)
    try:
        res = one.generate_batch([TEXT], params=[one.request_params(seed=7)])
        want, want_mu, pcm = one.batch_audio_with(0, loudness=-16.0), one.batch_audio_with(0, 8000, "mulaw", 1.25, -16.0), res[0]["pcm"]
        one.generate_long(LONG_TEXT, join=_pkg().join_params(gap_samples=600), params=one.request_params(seed=7))
        want_long = one.long_audio_with(loudness=-23.5)
    finally:
        one.free()
    assert _chunks(level)[b"data"] == want.tobytes() and len(want) == len(pcm) > 0
    assert _chunks(level_mu)[b"data"] == want_mu.tobytes()
    assert _chunks(long_level)[b"data"] == want_long.tobytes() and len(want_long) > 0


# ---- T6: refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    pkg = _pkg()
    lib, h = ctx._lib, ctx._h
    x = noise(12000, 0.1, 9)
    good = ctx.level_many([x], TARGET)[0]
    out = np.zeros(1 << 20, np.uint8)
    info = (pkg.BarkHipLoudnessInfo * 65)()
    z = np.zeros(16, np.float64)
    zp = z.ctypes.data_as(C.POINTER(C.c_double))

    def level(arrs, params, speeds=None, to=None, cap=out.size):
        ptrs = (C.c_void_p * len(arrs))(*[v.ctypes.data for v in arrs])
        ns = np.asarray([len(v) for v in arrs], np.int32)
        par = (pkg.BarkHipLoudnessParams * len(arrs))(*params)
        sp = None if speeds is None else np.asarray(speeds, np.int32).ctypes.data
        return lib.bark_hip_level_many(h, ptrs, ns.ctypes.data, len(arrs), par, sp, None if to is None else C.byref(to), out.ctypes.data, cap, None, info)

    def measure(arrs, params=None):
        ptrs = (C.c_void_p * len(arrs))(*[v.ctypes.data for v in arrs])
        ns = np.asarray([len(v) for v in arrs], np.int32)
        par = None if params is None else (pkg.BarkHipLoudnessParams * len(arrs))(*params)
        return lib.bark_hip_loudness_many(h, ptrs, ns.ctypes.data, len(arrs), par, info)

    ok = pkg.loudness_params(TARGET)
    assert level([x], [ok]) == 48000 and measure([x]) == 1 and measure([x], [ok]) == 1
    for t in (-4001, -499, 1, 1600, -1):
        assert level([x], [pkg.BarkHipLoudnessParams(t, 1.0, 10.0)]) == -1 and measure([x], [pkg.BarkHipLoudnessParams(t, 1.0, 10.0)]) == -1, t
    for t in (-4000, -500):
        assert level([x], [pkg.BarkHipLoudnessParams(t, 1.0, 10.0)]) == 48000, t
    for ceiling, cap in ((-1.0, 10.0), (1.0, -1.0), (math.inf, 10.0), (1.0, math.inf), (math.nan, 10.0), (1.0, math.nan)):
        assert level([x], [pkg.BarkHipLoudnessParams(-1600, ceiling, cap)]) == -1 and measure([x], [pkg.BarkHipLoudnessParams(-1600, ceiling, cap)]) == -1
    assert level([x], [pkg.BarkHipLoudnessParams(-1600, 0.0, 0.0)]) == 48000                  # no ceiling, no cap
    for bad in (np.nan, np.inf, -np.inf, 65520.0, -65520.0):
        y = x.copy(); y[1234] = bad
        assert level([x, y], [ok, ok]) == -1 and measure([y]) == -1 and lib.bark_hip_loudness_hops(h, y.ctypes.data, len(y), zp, 16) == -1, bad
    y = x.copy(); y[1234] = np.nextafter(np.float32(65520.0), np.float32(0.0))
    assert level([y], [ok]) == 48000 and info[0].peak == y[1234]
    assert level([x] * 65, [ok] * 65) == -1 and measure([x] * 65) == -1
    assert level([x], [ok], [2001]) == -1 and level([x], [ok], [499]) == -1 and level([x], [ok], [1250]) == 4 * 9600
    assert level([x], [ok], to=pkg.audio_format(11025, 0)) == -1 and level([x], [ok], to=pkg.audio_format(48000, 3)) == -1
    assert level([x], [ok], cap=47999) == -1 and level([x], [ok], cap=48000) == 48000
    assert level([np.zeros(lr.MAX_SAMPLES + 1, np.float32)], [ok]) == -1
    assert lib.bark_hip_loudness_hops(h, x.ctypes.data, len(x), zp, 4) == -1 and lib.bark_hip_loudness_hops(h, x.ctypes.data, len(x), zp, 5) == 5
    assert lib.bark_hip_loudness_hops(h, x.ctypes.data, 0, zp, 16) == -1 and lib.bark_hip_loudness_hops(h, x.ctypes.data, 2399, None, 0) == 0
    assert lib.bark_hip_time_loudness(h, 65, 1000, 0, 1) < 0 and lib.bark_hip_time_loudness(h, 1, 0, 1, 1) < 0
    assert ctx.time_loudness(2, 12000, False, 2) > 0.0 and ctx.time_loudness(2, 12000, True, 2) > 0.0
    with pytest.raises(ValueError):
        ctx.level_many([x], -3.0)
    with pytest.raises(ValueError):
        ctx.loudness(x[:0])
    _same("after the refusals", ctx.level_many([x], TARGET)[0], good)
    assert ctx.generate_audio(TEXT) and len(ctx.audio_data()) > 0                            # the context still generates
