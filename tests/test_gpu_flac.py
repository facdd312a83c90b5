"""GPU tests of the FLAC encoder (rule C18f): every byte the device writes against tests/flac_ref.py, and the per-frame choices
(subframe, partition order, length, CRC-16) against the reference's - on the lengths where the predictor order, the partition order or the frame count
changes, for the eight kinds of input that reach CONSTANT, VERBATIM, every FIXED order, small and mixed Rice parameters and the escape code; a ragged batch
of 64 in two orders; a result of 300 frames (more frames than the pack kernel has lanes); every rate's header; then the routes that render a held result
(audio_as / audio_with, batch_audio_with, long_audio_with, the request collector, bark_batch_server's "format": "flac") against the reference over the
same route's s16 bytes; the refusals; and one context through a small, a larger and a small call again.  Everything is an equality of bytes."""
import ctypes as C
import json
import os
import urllib.request

import numpy as np
import pytest

import flac_ref as fr

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "hello world this is bark"
LONG_TEXT = "hello world. this is bark"


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


_REF = {}


def ref(kind, n, rate=24000):
    """(samples, stream, [frame records]) of the reference, computed once per input"""
    key = (kind, n, rate)
    if key not in _REF:
        x = fr.signal(kind, n)
        frames = fr.encode_frames(x, rate)
        _REF[key] = (x, fr.encode(x, rate), np.asarray([i for _, i in frames], np.int32))
    return _REF[key]


def _same_bytes(what, got: bytes, want: bytes):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        k = min(len(a), len(b))
        bad = np.flatnonzero(a[:k] != b[:k])
        raise AssertionError(f"{what}: {len(a)} bytes against {len(b)}, first difference at {bad[:1]}")


@pytest.mark.parametrize("kind", fr.KINDS)
def test_streams_and_frame_choices_equal_the_reference(ctx, kind):
    """the fourteen lengths as one batch: the bytes, and what the reference's decoder makes of them; then the frame records length by length"""
    cases = [ref(kind, n) for n in fr.LENGTHS]
    got = ctx.flac_encode_many([x for x, _, _ in cases], 24000)
    for n, (x, want, frames), g in zip(fr.LENGTHS, cases, got):
        _same_bytes(f"{kind} {n}", g, want)
        y, rate = fr.decode(g)
        assert rate == 24000 and np.array_equal(x, y), (kind, n)
        rec = ctx.flac_frames(x, 24000)
        assert rec.tolist() == frames.tolist(), (kind, n, rec.tolist(), frames.tolist())


def test_the_inputs_reach_every_subframe_and_code(ctx):
    """what the device chose over all cases: CONSTANT, VERBATIM, each FIXED order, partition orders 0 .. 4"""
    recs = np.concatenate([ref(kind, n)[2] for kind in fr.KINDS for n in fr.LENGTHS] + [ref("sine_click", 4096 * k)[2] for k in (2, 3)])
    assert {0, 1, 8, 9, 10} <= set(recs[:, 0].tolist()), sorted(set(recs[:, 0].tolist()))
    assert set(recs[:, 1].tolist()) >= {0, 4}
    # orders 3 and 4: rounded sines, slow enough that the third or the fourth difference is the first to sink into the rounding noise
    t = np.arange(4096)
    for amp, w, code in ((1000.0, 0.05, 11), (30000.0, 0.3, 12)):
        x = np.round(amp * np.sin(w * t)).astype(np.int16)
        want = fr.encode_frames(x, 24000)
        assert want[0][1][0] == code
        assert ctx.flac_frames(x, 24000).tolist() == [want[0][1]] and ctx.flac_encode(x, 24000) == fr.encode(x, 24000)


def _ragged(order_seed):
    rng = np.random.default_rng(order_seed)
    pairs = [(fr.KINDS[i % len(fr.KINDS)], fr.LENGTHS[(i * 5 + i // 14) % len(fr.LENGTHS)]) for i in range(64)]
    return [pairs[i] for i in rng.permutation(64)]


def test_a_ragged_batch_of_64_equals_64_single_encodings(ctx):
    pairs = _ragged(3)
    assert len({n for _, n in pairs}) == len(fr.LENGTHS)
    for batch in (pairs, pairs[::-1]):
        got = ctx.flac_encode_many([ref(k, n)[0] for k, n in batch], 24000)
        for (k, n), g in zip(batch, got):
            _same_bytes(f"{k} {n} in a batch of 64", g, ref(k, n)[1])


def test_a_ragged_batch_of_5_equals_5_single_encodings(ctx):
    """the small form of the test above (the host-emulated engine runs this one)"""
    batch = [("sine_click", 4097), ("alternating", 17), ("loud_first_partition", 256), ("silence", 1), ("small_noise", 4095)]
    for order in (batch, batch[::-1]):
        for (k, n), g in zip(order, ctx.flac_encode_many([ref(k, n)[0] for k, n in order], 24000)):
            _same_bytes(f"{k} {n} in a batch of 5", g, ref(k, n)[1])


def test_a_result_of_300_frames(ctx):
    n = 300 * 4096 - 100
    x, want, frames = ref("small_noise", n)
    got = ctx.flac_encode_many([ref("sine_click", 17)[0], x, ref("ramp", 4097)[0]], 24000)
    _same_bytes("17 samples in front of 300 frames", got[0], ref("sine_click", 17)[1])
    _same_bytes("300 frames", got[1], want)
    _same_bytes("4097 samples behind 300 frames", got[2], ref("ramp", 4097)[1])
    assert len(frames) == 300 and ctx.flac_frames(x, 24000).tolist() == frames.tolist()


@pytest.mark.parametrize("rate", fr.RATES)
def test_every_rates_header(ctx, rate):
    x, want, frames = ref("sine_click", 4097, rate)
    _same_bytes(f"{rate} Hz", ctx.flac_encode(x, rate), want)
    assert fr.decode(want)[1] == rate


def test_one_context_through_a_small_a_larger_and_a_small_call():
    c = _load()
    try:
        for kind, n in (("sine_click", 255), ("loud_first_partition", 12289), ("small_noise", 40 * 4096 + 5), ("sine_click", 16), ("white", 4097)):
            _same_bytes(f"{kind} {n}", c.flac_encode(ref(kind, n)[0], 24000), ref(kind, n)[1])
    finally:
        c.free()


# ---- the routes ---------------------------------------------------------------------------------------------------------------------------------------------
def _flac_of(s16, rate):
    return fr.encode(np.asarray(s16, np.int16), rate)


def test_audio_as_and_audio_with_return_the_stream_of_the_routes_s16(ctx):
    pkg = _pkg()
    assert ctx.generate_audio(TEXT)
    for rate in (24000, 16000, 48000):
        _same_bytes(f"audio_as {rate}", ctx.audio_as(rate, "flac").tobytes(), _flac_of(ctx.audio_as(rate, "s16"), rate))
    _same_bytes("audio_at 1.25 at 8000", ctx.audio_at(1.25, 8000, "flac").tobytes(), _flac_of(ctx.audio_at(1.25, 8000, "s16"), 8000))
    got = ctx.audio_with(22050, "flac", 0.8, -16.0)
    s16 = ctx.audio_with(22050, "s16", 0.8, -16.0)
    _same_bytes("audio_with -16 LUFS at 0.8 and 22050", got.tobytes(), _flac_of(s16, 22050))
    y, rate = fr.decode(got.tobytes())
    assert rate == 22050 and np.array_equal(y, s16)
    # the capacity is checked against the real length
    to = pkg.audio_format(16000, "flac")
    want = _flac_of(ctx.audio_as(16000, "s16"), 16000)
    buf = np.zeros(len(want), np.uint8)
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(to), None, 0) == -2 - len(want)
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(to), buf.ctypes.data, len(want) - 1) == -2 - len(want)
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(to), buf.ctypes.data, len(want)) == len(want) and buf.tobytes() == want
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(pkg.audio_format(11025, "flac")), buf.ctypes.data, len(want)) == -1
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(pkg.audio_format(16000, 4)), buf.ctypes.data, len(want)) == -1


@pytest.mark.lock_step_job
def test_batch_audio_with_and_long_audio_with(ctx):
    pkg = _pkg()
    res = ctx.generate_batch([TEXT, "another one"])
    assert all(r is not None for r in res)
    for i in range(2):
        _same_bytes(f"batch_audio_as {i}", ctx.batch_audio_as(i, 32000, "flac").tobytes(), _flac_of(ctx.batch_audio_as(i, 32000, "s16"), 32000))
        _same_bytes(f"batch_audio_with {i}", ctx.batch_audio_with(i, 12000, "flac", 1.25, -23.0).tobytes(), _flac_of(ctx.batch_audio_with(i, 12000, "s16", 1.25, -23.0), 12000))
    join = pkg.join_params(gap_samples=600, fade_samples=48, trim_threshold=0.02)
    chunks = ctx.generate_long(LONG_TEXT, join=join, params=ctx.request_params(seed=5))
    assert len(chunks) == 2
    for rate, speed, loud in ((24000, 1.0, None), (44100, 1.0, None), (16000, 1.25, None), (24000, 0.8, -16.0)):
        got = ctx.long_audio_with(rate, "flac", speed, loud)
        s16 = ctx.long_audio_with(rate, "s16", speed, loud)
        _same_bytes(f"long_audio_with {rate} {speed} {loud}", got.tobytes(), _flac_of(s16, rate))
    _same_bytes("long_audio_as", ctx.long_audio_as(16000, "flac").tobytes(), _flac_of(ctx.long_audio_as(16000, "s16"), 16000))
    _same_bytes("long_audio_at", ctx.long_audio_at(1.25, 8000, "flac").tobytes(), _flac_of(ctx.long_audio_at(1.25, 8000, "s16"), 8000))
    y, rate = fr.decode(ctx.long_audio_as(16000, "flac").tobytes())
    assert rate == 16000 and np.array_equal(y, ctx.long_audio_as(16000, "s16"))


@pytest.mark.concurrency
def test_collector_serves_flac_beside_other_formats(ctx):
    pkg = _pkg()
    texts = [TEXT, "another one", "third", "and a fourth", "a fifth"]
    fmts = [pkg.audio_format(24000, "flac"), None, pkg.audio_format(8000, "flac"), pkg.audio_format(48000, "s16"), pkg.audio_format(24000, "flac")]
    speeds = [None, None, 1.25, None, None]
    louds = [None, None, -23.0, None, -16.0]
    join = pkg.join_params(gap_samples=600)
    owner = _load(temp=0.7, fine_temp=0.5)
    try:
        with pkg.Batcher(owner, max_batch=8, max_wait_ms=200) as b:
            tickets = [b.submit(t, seed=40 + i, audio_format=f, speed=s, loudness=l) for i, (t, f, s, l) in enumerate(zip(texts, fmts, speeds, louds))]
            plain = [b.submit(t, seed=40 + i) for i, t in enumerate(texts)]                  # the same requests in the engine's own form
            long_flac = b.submit(LONG_TEXT, seed=60, long=pkg.BarkHipLongParams(0, 0, join), audio_format=pkg.audio_format(16000, "flac"))
            got = [b.wait_bytes(t) for t in tickets]
            pcm = [b.wait(t) for t in plain]
            got_long = b.wait_bytes(long_flac)
            assert b._lib.bark_hip_batcher_submit_as(b._b, b"x", None, None, None, C.byref(pkg.audio_format(11025, "flac"))) == -1
            assert b._lib.bark_hip_batcher_submit_as(b._b, b"x", None, None, None, C.byref(pkg.audio_format(24000, 4))) == -1
        owner.generate_long(LONG_TEXT, join=join, params=owner.request_params(seed=60))
        want_long = _flac_of(owner.long_audio_as(16000, "s16"), 16000)
    finally:
        owner.free()
    _same_bytes("request 0", got[0].tobytes(), _flac_of(ctx.resample_many([pcm[0]], 24000, 24000, "s16")[0], 24000))
    assert got[1].dtype == np.float32 and got[1].tobytes() == pcm[1].tobytes()
    _same_bytes("request 2 at -23 LUFS, 1.25, 8000", got[2].tobytes(), _flac_of(ctx.level_many([pcm[2]], -23.0, [1.25], 8000, "s16")[0], 8000))
    assert got[3].tobytes() == ctx.resample_many([pcm[3]], 24000, 48000, "s16")[0].tobytes()
    _same_bytes("request 4 at -16 LUFS", got[4].tobytes(), _flac_of(ctx.level_many([pcm[4]], -16.0, None, 24000, "s16")[0], 24000))
    _same_bytes("the long text", got_long.tobytes(), want_long)
    assert len(got_long) > 42


@pytest.mark.concurrency
def test_native_batch_server_flac_format():
    from test_gpu_output_format import _chunks
    from test_gpu_voice_from_audio import _Server
    model = _model("toy")

    def post(srv, fields):
        req = urllib.request.Request(f"http://127.0.0.1:{srv.port}/bark", data=json.dumps(fields).encode(), method="POST")
        with urllib.request.urlopen(req, timeout=200) as r:
            return r.status, r.headers.get("Content-Type"), r.read()
    with _Server("-m", model) as srv:
        st, kind, flac = post(srv, {"text": TEXT, "seed": 7, "format": "flac", "sample_rate": 16000, "speed": 1.25, "loudness": -16})
        assert st == 200 and kind == "audio/flac"
        st, kind, wav = post(srv, {"text": TEXT, "seed": 7, "format": "s16", "sample_rate": 16000, "speed": 1.25, "loudness": -16})
        assert st == 200 and kind == "audio/wav"
        st, kind, long_flac = post(srv, {"text": LONG_TEXT, "seed": 7, "format": "flac", "long": True, "gap_ms": 25})
        assert st == 200 and kind == "audio/flac"
        st, kind, long_wav = post(srv, {"text": LONG_TEXT, "seed": 7, "format": "s16", "long": True, "gap_ms": 25})
        assert st == 200
        for bad in ("FLAC", "ogg", 3, True):
            assert srv.request("POST", "/bark", json.dumps({"text": TEXT, "format": bad}).encode())[0] == 400, bad
    with _Server("-m", model, "--format", "flac", "--sample-rate", "16000") as srv:
        st, kind, flac2 = post(srv, {"text": TEXT, "seed": 7, "speed": 1.25, "loudness": -16})
        assert st == 200 and kind == "audio/flac" and flac2 == flac
    _same_bytes("the server's stream", flac, _flac_of(np.frombuffer(_chunks(wav)[b"data"], "<i2"), 16000))
    _same_bytes("the server's long stream", long_flac, _flac_of(np.frombuffer(_chunks(long_wav)[b"data"], "<i2"), 24000))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    pkg = _pkg()
    lib = ctx._lib
    x = ref("sine_click", 4097)[0]
    out = np.zeros(fr.max_bytes(len(x)), np.uint8)
    lengths = np.zeros(64, np.int32)

    def many(xs, rate=24000, cap=None, count=None, h=None):
        ptrs = (C.c_void_p * max(len(xs), 1))(*[None if v is None else v.ctypes.data for v in xs])
        ns = np.asarray([0 if v is None else len(v) for v in xs], np.int32)
        return lib.bark_hip_flac_encode_many(ctx._h if h is None else h, ptrs, ns.ctypes.data, len(xs) if count is None else count, rate, out.ctypes.data,
                                             out.size if cap is None else cap, lengths.ctypes.data)
    want = ref("sine_click", 4097)[1]
    assert many([x]) == len(want) and out[:len(want)].tobytes() == want and lengths[0] == len(want)
    assert many([x], count=0) == -1 and many([x] * 65) == -1 and many([x, None]) == -1
    assert many([x], rate=11025) == -1 and many([x], rate=0) == -1 and many([x], rate=96000) == -1
    assert many([x[:0]]) == -1
    assert lib.bark_hip_flac_encode_many(None, None, None, 1, 24000, out.ctypes.data, out.size, None) == -1
    assert lib.bark_hip_flac_encode_many(ctx._h, None, None, 1, 24000, out.ctypes.data, out.size, None) == -1
    assert many([x], cap=len(want) - 1) == -2 - len(want) and many([x], cap=0) == -2 - len(want)        # too small: the needed size
    rec = np.zeros(8, np.int32)
    assert lib.bark_hip_flac_frames(ctx._h, x.ctypes.data, len(x), 24000, rec.ctypes.data, 1) == -1      # two frames, room for one record
    assert lib.bark_hip_flac_frames(ctx._h, x.ctypes.data, len(x), 24000, None, 2) == -1
    assert lib.bark_hip_flac_frames(ctx._h, x.ctypes.data, len(x), 24000, rec.ctypes.data, 2) == 2
    assert lib.bark_hip_time_flac(ctx._h, 0, 4096, 1) < 0 and lib.bark_hip_time_flac(ctx._h, 65, 4096, 1) < 0 and lib.bark_hip_time_flac(None, 1, 4096, 1) < 0
    assert lib.bark_hip_time_flac_launch(ctx._h, 1, 4096, 0, 1) < 0
    assert ctx.time_flac(2, 5000, iters=2) > 0.0 and ctx.time_flac(2, 5000, iters=2, which=1) > 0.0 and ctx.time_flac(2, 5000, iters=2, which=2) > 0.0
    with pytest.raises(ValueError):
        ctx.flac_encode(x, 11025)
    # the calls on caller audio keep refusing the container
    f = np.zeros(100, np.float32)
    with pytest.raises(ValueError):
        ctx.resample_many([f], 24000, 24000, "flac")
    assert ctx.flac_encode(x, 24000) == want
