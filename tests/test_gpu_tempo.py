"""GPU tests of the speaking rate per request (rule C16t): the time-scale kernel bit for bit against tests/tempo_ref.py with the
library's own window table - samples and chosen positions, ragged batches of mixed speeds with speed 1000 riding along - ragged batches against single
calls, every rate and format behind the tempo, the refusals, the routes that time-scale a generation (audio_at, batch_audio_at, long_audio_at, the request
collector) and bark_batch_server's "speed" field.  Everything here is an equality of bits or bytes."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import output_format_ref as ofr
import resample_ref as rr
import tempo_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "hello world this is bark"
LONG_TEXT = "hello world. this is bark speech! go there? yes"
FORMATS = (("f32", ofr.F32), ("s16", ofr.S16), ("mulaw", ofr.MULAW))
EDGE_LENGTHS = [1, 2, 359, 360, 361, 719, 720, 721, 1081]                  # around one hop, one frame and a frame and a half
SEEDED_LENGTHS = sorted(int(v) for v in np.random.default_rng(16).integers(1082, 3001, 5)) + [6000]      # five seeded ones and the longest
SPEEDS = [500, 667, 999, 1001, 1250, 1500, 2000]
KINDS = ["dense", "tone", "silence", "impulse", "constant", "loud"]


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
def window():
    """the library's own window table"""
    w = np.zeros(tr.W, np.float32)
    assert _pkg().load_library().bark_hip_tempo_window(w.ctypes.data) == tr.W
    return w


@pytest.fixture(scope="module")
def tables():
    """the library's own resampler table of every output rate, [L][2 HALF]"""
    lib = _pkg().load_library()
    out = {}
    for rate in ofr.RATES:
        if rate == 24000:
            continue
        lmh = np.zeros(3, np.int32)
        n = lib.bark_hip_resample_table(24000, rate, None, 0, lmh.ctypes.data)
        h = np.zeros(n, np.float32)
        assert lib.bark_hip_resample_table(24000, rate, h.ctypes.data, n, lmh.ctypes.data) == n
        out[rate] = h.reshape(int(lmh[0]), 2 * int(lmh[2]))
    return out


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:5]]} != {want.reshape(-1)[bad[:5]]}"


def signal(kind: str, n: int) -> np.ndarray:
    if kind == "dense":
        return rr.dense_signal(n, seed=n)
    if kind == "tone":                                                      # period 48 samples: 240 = 5 periods, so candidates a period apart score within roundings
        return (0.5 * np.sin(2.0 * np.pi * np.arange(n) / 48.0)).astype(np.float32)
    if kind == "silence":
        return np.zeros(n, np.float32)
    if kind == "impulse":
        x = np.zeros(n, np.float32); x[(2 * n) // 3] = 1.0
        return x
    if kind == "constant":
        return np.full(n, 0.25, np.float32)
    assert kind == "loud"
    return np.random.default_rng([n, 16]).uniform(-65000.0, 65000.0, n).astype(np.float32)


def _cases(group):
    """(kind, n, p) of a group: the edge lengths in dense noise at every speed (two groups), or one kind of signal at every speed over the seeded lengths"""
    if group == "edges_slow":
        return [("dense", n, p) for n in EDGE_LENGTHS for p in SPEEDS[:3]]
    if group == "edges_fast":
        return [("dense", n, p) for n in EDGE_LENGTHS for p in SPEEDS[3:]]
    i = KINDS.index(group)
    return [(group, SEEDED_LENGTHS[(i + j) % 6], p) for j, p in enumerate(SPEEDS)]


GROUPS = ["edges_slow", "edges_fast"] + KINDS
_REF = {}


def reference(kind, n, p, window):
    """(y, pos) of the rule, computed once per case and shared by the tests"""
    key = (kind, n, p)
    if key not in _REF:
        _REF[key] = tr.tempo(signal(kind, n), p, window, want_pos=True)
    return _REF[key]


def test_the_cases_stay_near_500_frames():
    frames = sum(tr.n_frames(n, p) for g in GROUPS for _, n, p in _cases(g))
    assert 300 <= frames <= 560, frames


# ---- T1: the kernel against the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_kernel_is_c16t_bit_for_bit(ctx, window, group):
    """a group travels as ragged batches of mixed speeds, every third case followed by a copy at speed 1000 (it must come back unchanged); positions come from single calls"""
    cases = _cases(group)
    xs, ps = [], []
    for k, (kind, n, p) in enumerate(cases):
        xs.append(signal(kind, n)); ps.append(p)
        if k % 3 == 0:
            xs.append(signal(kind, n)); ps.append(1000)
    got = []
    for b in range(0, len(xs), 64):
        got += ctx.tempo_many(xs[b:b + 64], [p / 1000.0 for p in ps[b:b + 64]])
    seen = 0
    for x, p, g in zip(xs, ps, got):
        if p == 1000:
            assert g.tobytes() == x.tobytes()
            continue
        kind, n, _ = cases[seen]; seen += 1
        y, pos = reference(kind, n, p, window)
        assert len(g) == tr.out_len(n, p) == ctx._lib.bark_hip_tempo_out_len(n, p)
        _same(f"{kind} n={n} p={p} positions", ctx.tempo_positions(x, p / 1000.0), pos)
        _same(f"{kind} n={n} p={p}", g, y)
        if kind == "silence":
            assert pos.tolist() == [tr.nominal(k, p) for k in range(len(pos))] and not g.any()
    assert seen == len(cases)
    x = signal("dense", 721)
    _same("positions at speed 1000", ctx.tempo_positions(x, 1.0), np.arange(3, dtype=np.int32) * tr.HS)


# ---- T2: ragged batches ----------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batches_equal_single_calls_and_the_scratch_is_reused(ctx, window):
    cases = _cases("edges_fast")[:12] + _cases("dense")[:3] + _cases("tone")[:2]
    xs = [signal(kind, n) for kind, n, _ in cases]
    ps = [p / 1000.0 for _, _, p in cases]
    big = rr.dense_signal(40000, seed=5)
    single = [ctx.tempo(x, p) for x, p in zip(xs, ps)]
    for (kind, n, p), g in zip(cases, single):
        _same(f"single {kind} n={n} p={p}", g, reference(kind, n, p, window)[0])
    first_big = ctx.tempo(big, 0.75)                                                          # grows every buffer ..
    for count in (1, 2, 7, len(xs)):                                                          # .. which the smaller calls behind it reuse
        got = ctx.tempo_many(xs[:count], ps[:count])
        assert len(got) == count
        for k in range(count):
            _same(f"count {count} segment {k}", got[k], single[k])
    pad = [np.zeros(1, np.float32)] * (64 - len(xs))
    got = ctx.tempo_many(pad + xs, [1.0] * len(pad) + ps)                                     # 64 segments, the first ones a sample long at speed 1000
    for k in range(len(xs)):
        _same(f"64 segments, segment {k}", got[len(pad) + k], single[k])
    _same("the long one again", ctx.tempo(big, 0.75), first_big)
    assert len(first_big) == tr.out_len(40000, 750)


# ---- T3: every rate and format behind the tempo ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", ofr.RATES)
def test_every_rate_and_format_behind_the_tempo(ctx, window, tables, rate):
    kind, n, p = "dense", 1081, 1250
    x = signal(kind, n)
    y = reference(kind, n, p, window)[0]
    for name, fmt in FORMATS:
        want = ofr.to_format(ofr.resample(y, 24000, rate, h=tables.get(rate)), fmt)
        got = ctx.tempo_many([x, x[:400]], [p / 1000.0, 1.0], rate, name)
        _same(f"{rate} {name}", got[0], want)
        _same(f"{rate} {name}, the segment at speed 1000", got[1], ofr.to_format(ofr.resample(x[:400], 24000, rate, h=tables.get(rate)), fmt))


# ---- T4: refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    pkg = _pkg()
    lib, h = ctx._lib, ctx._h
    x = rr.dense_signal(3000)
    good = ctx.tempo(x, 1.25)
    out = np.zeros(1 << 20, np.uint8)
    n_out = np.zeros(4, np.int32)
    pos = np.zeros(64, np.int32)

    def one(arr, n, p=1250, cap=out.size // 4):
        return lib.bark_hip_tempo(h, None if arr is None else arr.ctypes.data, n, p, out.ctypes.data, cap)

    def many(arrs, speeds, to=None, cap=out.size):
        ptrs = (C.c_void_p * len(arrs))(*[v.ctypes.data for v in arrs])
        ns = np.asarray([len(v) for v in arrs], np.int32)
        sp = np.asarray(speeds, np.int32)
        return lib.bark_hip_tempo_many(h, ptrs, ns.ctypes.data, len(arrs), sp.ctypes.data, None if to is None else C.byref(to), out.ctypes.data, cap, n_out.ctypes.data)

    assert one(x, len(x), 499) == -1 and one(x, len(x), 2001) == -1 and one(x, len(x), 0) == -1 and one(x, len(x), -1000) == -1
    assert one(x, 0) == -1 and one(x, -3) == -1 and one(None, 10) == -1
    assert one(np.zeros(tr.MAX_SAMPLES + 1, np.float32), tr.MAX_SAMPLES + 1) == -1
    for bad in (np.nan, np.inf, -np.inf, 65520.0, -65520.0):
        y = x.copy(); y[1234] = bad
        assert one(y, len(y)) == -1 and many([x, y], [1250, 1000]) == -1 and lib.bark_hip_tempo_positions(h, y.ctypes.data, len(y), 1250, pos.ctypes.data, 64) == -1, bad
    y = x.copy(); y[1234] = np.nextafter(np.float32(65520.0), np.float32(0.0))
    assert one(y, len(y)) == 2400
    assert one(x, len(x), cap=2399) == -1 and one(x, len(x), cap=2400) == 2400                # capacity in floats
    s16 = pkg.audio_format(48000, "s16")
    assert many([x], [1250], s16, cap=9599) == -1 and many([x], [1250], s16, cap=9600) == 9600 and int(n_out[0]) == 4800      # one byte short
    assert many([x], [1250], cap=9599) == -1 and many([x], [1250], cap=9600) == 9600
    assert many([x] * 65, [1250] * 65) == -1 and many([x, x], [1250, 2001]) == -1 and many([x], [1250], pkg.audio_format(11025, 0)) == -1
    assert many([x], [1250], pkg.audio_format(48000, 3)) == -1
    assert lib.bark_hip_tempo_positions(h, x.ctypes.data, len(x), 1250, pos.ctypes.data, 6) == -1      # 7 frames
    assert lib.bark_hip_tempo_positions(h, x.ctypes.data, len(x), 1250, pos.ctypes.data, 7) == 7
    assert lib.bark_hip_tempo(None, x.ctypes.data, 10, 1250, out.ctypes.data, 100) == -1
    assert lib.bark_hip_time_tempo(h, 65, 1000, 1250, 1) < 0 and lib.bark_hip_time_tempo(h, 1, 1000, 1000, 1) < 0 and ctx.time_tempo(2, 3000, 1.25, 2) > 0.0
    with pytest.raises(ValueError):
        ctx.tempo(x, 2.5)
    with pytest.raises(ValueError):
        ctx.tempo(x[:0], 1.25)
    _same("after the refusals", ctx.tempo(x, 1.25), good)
    assert ctx.generate_audio(TEXT) and len(ctx.audio_data()) > 0                            # the context still generates


# ---- T5: the routes on the toy model -------------------------------------------------------------------------------------------------------------------------
def test_audio_at_and_batch_audio_at_are_the_rule_over_the_result(ctx, window, tables):
    assert ctx.generate_audio(TEXT)
    pcm = np.asarray(ctx.audio_data(), np.float32).copy()
    want = tr.tempo(pcm, 1250, window)
    _same("audio_at 1.25", ctx.audio_at(1.25), want)
    _same("audio_at 1.25 at 8000 mu-law", ctx.audio_at(1.25, 8000, "mulaw"), ofr.to_format(ofr.resample(want, 24000, 8000, h=tables[8000]), ofr.MULAW))
    for rate, name in ((24000, "f32"), (48000, "s16"), (8000, "mulaw")):
        assert ctx.audio_at(1.0, rate, name).tobytes() == ctx.audio_as(rate, name).tobytes()
    assert np.asarray(ctx.audio_data(), np.float32).tobytes() == pcm.tobytes()
    to = _pkg().audio_format(16000, "s16")
    nb = 2 * ofr.n_out(tr.out_len(len(pcm), 1250), 24000, 16000)
    buf = np.zeros(nb, np.uint8)
    assert ctx._lib.bark_hip_get_audio_at(ctx._h, C.byref(to), 1250, buf.ctypes.data, nb - 1) == -2 - nb                     # too small: -(2 + bytes)
    assert ctx._lib.bark_hip_get_audio_at(ctx._h, C.byref(to), 1250, buf.ctypes.data, nb) == nb
    assert ctx._lib.bark_hip_get_audio_at(ctx._h, C.byref(to), 2001, buf.ctypes.data, nb) == -1
    assert ctx._lib.bark_hip_get_audio_at(ctx._h, C.byref(_pkg().audio_format(11025, "s16")), 1250, buf.ctypes.data, nb) == -1
    res = ctx.generate_batch([TEXT, "another one"])
    assert all(r is not None for r in res)
    for i, r in enumerate(res):
        _same(f"batch_audio_at {i}", ctx.batch_audio_at(i, 1.25), tr.tempo(r["pcm"], 1250, window))
        assert ctx.batch_audio_at(i, 1.0, 48000, "s16").tobytes() == ctx.batch_audio_as(i, 48000, "s16").tobytes()
        _same(f"batch_audio_at {i} 0.8 at 44100 s16", ctx.batch_audio_at(i, 0.8, 44100, "s16"), ctx.tempo_many([r["pcm"]], [0.8], 44100, "s16")[0])
    assert ctx._lib.bark_hip_batch_audio_at(ctx._h, 2, C.byref(to), 1250, buf.ctypes.data, nb) == -1


@pytest.mark.lock_step_job
def test_long_audio_at_is_the_join_of_the_tempo_of_each_chunk(ctx):
    pkg = _pkg()
    join = pkg.join_params(gap_samples=600, fade_samples=48)
    chunks = ctx.generate_long(LONG_TEXT, join=join, params=ctx.request_params(seed=5))
    assert len(chunks) == 4
    fast = ctx.tempo_many([c["pcm"] for c in chunks], [1.25] * len(chunks))
    for rate, name in ((24000, "f32"), (16000, "s16")):
        _same(f"long_audio_at {rate} {name}", ctx.long_audio_at(1.25, rate, name), ctx.join_many(fast, join, rate, name))
        assert ctx.long_audio_at(1.0, rate, name).tobytes() == ctx.long_audio_as(rate, name).tobytes()
        _same(f"long_audio_at {rate} {name} once more", ctx.long_audio_at(1.25, rate, name), ctx.join_many(fast, join, rate, name))
    assert ctx._lib.bark_hip_long_audio_at(ctx._h, None, 499, None, 0) == -1


@pytest.mark.concurrency
def test_collector_requests_at_a_speaking_rate(ctx, window):
    pkg = _pkg()
    texts = [TEXT, "another one", "third", "and a fourth"]
    speeds = [1.25, None, 0.8, 1.0]
    fmts = [None, None, pkg.audio_format(8000, "mulaw"), pkg.audio_format(48000, "s16")]
    join = pkg.join_params(gap_samples=600)
    owner = _load(temp=0.7, fine_temp=0.5)
    try:
        with pkg.Batcher(owner, max_batch=8, max_wait_ms=200) as b:
            tickets = [b.submit(t, seed=40 + i, audio_format=f, speed=s) for i, (t, s, f) in enumerate(zip(texts, speeds, fmts))]
            plain = [b.submit(t, seed=40 + i) for i, t in enumerate(texts)]                  # the same requests in the engine's own form
            long_fast = b.submit(LONG_TEXT, seed=60, long=pkg.BarkHipLongParams(0, 0, join), speed=1.25)
            got = [b.wait_bytes(t) for t in tickets]
            ref = [b.wait(t) for t in plain]
            got_long = b.wait_bytes(long_fast)
            assert b._lib.bark_hip_batcher_submit_at(b._b, b"x", None, None, None, None, 2001) == -1
            assert b._lib.bark_hip_batcher_submit_long_at(b._b, b"x. y", None, None, None, None, None, 499) == -1
        owner.generate_long(LONG_TEXT, join=join, params=owner.request_params(seed=60))
        want_long = owner.long_audio_at(1.25)
    finally:
        owner.free()
    _same("request 0 at 1.25", got[0], tr.tempo(ref[0], 1250, window))
    assert got[1].dtype == np.float32 and got[1].tobytes() == ref[1].tobytes()
    _same("request 2 at 0.8 in 8000 mu-law", got[2], ctx.tempo_many([ref[2]], [0.8], 8000, "mulaw")[0])
    _same("request 3 at 1.0 in 48000 s16", got[3], ctx.resample_many([ref[3]], 24000, 48000, fmt="s16")[0])
    _same("the long text at 1.25", got_long, want_long)
    assert len(got_long) > 0


# ---- T6: the server ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.concurrency
def test_native_batch_server_speed_field():
    from test_gpu_output_format import _chunks
    from test_gpu_voice_from_audio import _Server
    model = _model("toy")
    with _Server("-m", model) as srv:
        st, fast = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7, "speed": 1.25}).encode())
        assert st == 200
        st, fast_mu = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7, "speed": 1.25, "sample_rate": 8000, "format": "mulaw"}).encode())
        assert st == 200
        st, plain = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7}).encode())
        assert st == 200
        st, unit = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7, "speed": 1.0}).encode())
        assert st == 200 and unit == plain
        st, long_fast = srv.request("POST", "/bark", json.dumps({"text": LONG_TEXT, "seed": 7, "speed": 0.8, "long": True, "gap_ms": 25}).encode())
        assert st == 200
        for bad in (3, 0.49, 2.001, "fast", True, -1):
            assert srv.request("POST", "/bark", json.dumps({"text": TEXT, "speed": bad}).encode())[0] == 400, bad
    with _Server("-m", model, "--speed", "1.25") as srv:
        st, fast2 = srv.request("POST", "/bark", json.dumps({"text": TEXT, "seed": 7}).encode())
        assert st == 200 and fast2 == fast
    one = _load(n_steps_text_encoder=768)
    try:
        res = one.generate_batch([TEXT], params=[one.request_params(seed=7)])
        want, want_mu, pcm = one.batch_audio_at(0, 1.25), one.batch_audio_at(0, 1.25, 8000, "mulaw"), res[0]["pcm"]
        one.generate_long(LONG_TEXT, join=_pkg().join_params(gap_samples=600), params=one.request_params(seed=7))
        want_long = one.long_audio_at(0.8)
    finally:
        one.free()
    ch = _chunks(plain)
    assert ch[b"data"] == pcm.tobytes() and len(pcm) > 0
    ch = _chunks(fast)
    assert struct.unpack("<HHIIHH", ch[b"fmt "]) == (3, 1, 24000, 96000, 4, 32) and ch[b"data"] == want.tobytes() and len(want) == tr.out_len(len(pcm), 1250)
    ch = _chunks(fast_mu)
    assert struct.unpack("<I", ch[b"fact"]) == (len(want_mu),) and ch[b"data"] == want_mu.tobytes()
    assert _chunks(long_fast)[b"data"] == want_long.tobytes() and len(want_long) > 0
