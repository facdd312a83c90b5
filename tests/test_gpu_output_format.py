"""GPU tests of the output rate and sample format per request (rule C14r): the rational resampler kernel bit for bit against
tests/output_format_ref.py with the library's own table, the s16 and mu-law epilogues, ragged batches against single calls, the identity, the refusals, the
old 24 kHz -> 16 kHz kernel beside the new one, the routes that convert a generation (get_audio_as, batch_audio_as, the request collector) and
bark_batch_server's "sample_rate" / "format" fields and POST /voices?resample=1.  Everything here is an equality of bits or bytes."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import codec_encoder_ref as cref
import output_format_ref as ofr
import resample_ref as rr

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "hello world this is bark"
PAIR_IDS = [f"{a}-{b}-" for a, b in ofr.PAIRS]
FORMATS = (("f32", ofr.F32), ("s16", ofr.S16), ("mulaw", ofr.MULAW))
# every n in 1 .. 64, then 24 seeded lengths up to 20 011: several tiles of the kernel's 1024 outputs (and of any tile up to 4096) for every pair
LENGTHS = list(range(1, 65)) + sorted(int(v) for v in np.random.default_rng(14).integers(65, 20011, 23)) + [20011]


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
def tables():
    """the library's own table of every pair, [L][2 HALF]"""
    lib = _pkg().load_library()
    out = {}
    for a, b in ofr.PAIRS:
        lmh = np.zeros(3, np.int32)
        n = lib.bark_hip_resample_table(a, b, None, 0, lmh.ctypes.data)
        assert n > 0 and tuple(int(v) for v in lmh) == ofr.lmh(a, b)
        h = np.zeros(n, np.float32)
        assert lib.bark_hip_resample_table(a, b, h.ctypes.data, n, lmh.ctypes.data) == n
        out[(a, b)] = h.reshape(int(lmh[0]), 2 * int(lmh[2]))
    return out


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:5]]} != {want.reshape(-1)[bad[:5]]}"


def _want(x, pair, tables, fmt=ofr.F32):
    return ofr.to_format(ofr.resample(x, *pair, h=tables[pair]), fmt)


# ---- O1: the kernel against the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ofr.PAIRS, ids=PAIR_IDS)
def test_kernel_is_c14r_bit_for_bit(ctx, tables, pair):
    """all the lengths of a pair travel as ragged batches of 64 and 24 segments (test_ragged_batches_equal_single_calls ties those to single calls), the
    longest ones once more as single calls"""
    xs = [rr.dense_signal(n, seed=n) for n in LENGTHS]
    got = ctx.resample_many(xs[:64], *pair) + ctx.resample_many(xs[64:], *pair)
    for n, x, g in zip(LENGTHS, xs, got):
        assert len(g) == ofr.n_out(n, *pair)
        _same(f"{pair} n={n}", g, _want(x, pair, tables))
    for x in xs[-2:]:
        _same(f"{pair} single n={len(x)}", ctx.resample(x, *pair), _want(x, pair, tables))


# ---- O2: formats ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ofr.PAIRS, ids=PAIR_IDS)
def test_impulses_and_a_saturating_square_wave_in_every_format(ctx, tables, pair):
    n = 2500
    sigs = []
    for pos in (0, n // 2 + 1, n - 1):
        x = np.zeros(n, np.float32); x[pos] = 1.0
        sigs.append(x)
    sigs.append(np.where((np.arange(n) // 7) % 2 == 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32))       # full scale: overshoots, s16 saturates
    y = ofr.resample(sigs[3], *pair, h=tables[pair])
    assert np.abs(y).max() > 1.0 and {-32768, 32767} <= set(ofr.to_s16(y).tolist())
    for name, fmt in FORMATS:
        got = ctx.resample_many(sigs, *pair, fmt=name)
        for k, (x, g) in enumerate(zip(sigs, got)):
            _same(f"{pair} {name} signal {k}", g, _want(x, pair, tables, fmt))


def test_every_s16_value_through_mulaw_and_the_s16_ties(ctx):
    """through the format kernel alone (24000 -> 24000 runs no filter): every s16 value as s / 32768 exactly, and the ties of rintf"""
    s = np.arange(-32768, 32768).astype(np.int16)
    x = s.astype(np.float32) / np.float32(32768.0)
    _same("s16 of every value", ctx.resample_many([x], 24000, 24000, fmt="s16")[0], s)
    got = ctx.resample_many([x], 24000, 24000, fmt="mulaw")[0]
    _same("mu-law of every s16 value", got, ofr.mulaw_of_s16(s))
    assert [int(got[32768 + v]) for v in (0, -1, 32767, -32768)] == [0xFF, 0x7F, 0x80, 0x00]
    lsb = np.float32(1.0 / 32768.0)
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32766.5, 32767.5, -32768.5, 1e6, -1e6], np.float32) * lsb
    got = ctx.resample_many([ties], 24000, 24000, fmt="s16")[0]
    assert got.tolist() == [0, 2, 2, 0, -2, -2, 32766, 32767, -32768, 32767, -32768]
    _same("ties", got, ofr.to_s16(ties))
    _same("ties, mu-law", ctx.resample_many([ties], 24000, 24000, fmt="mulaw")[0], ofr.to_format(ties, ofr.MULAW))


# ---- O3: ragged batches --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(24000, 8000), (24000, 44100), (44100, 24000), (24000, 16000), (22050, 24000)], ids=lambda p: f"{p[0]}-{p[1]}-")
def test_ragged_batches_equal_single_calls(ctx, tables, pair):
    half = ofr.lmh(*pair)[2]
    lens = [1, half, 3, 1029, 2 * half + 1, 7, 4097, 2, 1500]                               # odd lengths: every later segment starts at an odd offset
    lens += [int(v) for v in np.random.default_rng(3).integers(1, 700, 64 - len(lens))]
    xs = [rr.dense_signal(n, seed=100 + k) for k, n in enumerate(lens)]
    for name, fmt in FORMATS:
        single = [ctx.resample_many([x], *pair, fmt=name)[0] for x in xs[:9]]
        for count in (1, 2, 9, 64):
            got = ctx.resample_many(xs[:count], *pair, fmt=name)
            assert len(got) == count
            for k in range(min(count, 9)):
                _same(f"{pair} {name} count {count} segment {k}", got[k], single[k])
        if fmt == ofr.F32:
            for k in range(9):
                _same(f"{pair} resample() segment {k}", ctx.resample(xs[k], *pair), single[k])
    got = ctx.resample_many(xs, *pair)                                                        # the segments behind the ninth against the rule itself
    for k in range(9, 64):
        _same(f"{pair} segment {k} of 64", got[k], _want(xs[k], pair, tables))


# ---- O4: identity, refusals, the old kernel ---------------------------------------------------------------------------------------------------------------
def test_identity_passes_the_bytes_on(ctx):
    x = np.random.default_rng(8).standard_normal(4099).astype(np.float32)
    x[:4] = [0.0, -0.0, 1e-42, -3e38]                                                        # signed zero, a denormal, a huge one
    assert ctx.resample(x, 24000, 24000).tobytes() == x.tobytes()
    got = ctx.resample_many([x, x[:1], x[5:]], 24000, 24000)
    assert [g.tobytes() for g in got] == [x.tobytes(), x[:1].tobytes(), x[5:].tobytes()]


def test_refusals_leave_the_context_usable(ctx):
    pkg = _pkg()
    lib, h = ctx._lib, ctx._h
    x = rr.dense_signal(3000)
    good = ctx.resample(x, 24000, 16000)
    out = np.zeros(1 << 20, np.uint8)
    n_out = np.zeros(4, np.int32)

    def one(arr, n, a=24000, b=16000, cap=out.size // 4):
        return lib.bark_hip_resample(h, None if arr is None else arr.ctypes.data, n, a, b, out.ctypes.data, cap)

    def many(arrs, to, a=24000, cap=out.size, lens=None):
        ptrs = (C.c_void_p * len(arrs))(*[v.ctypes.data for v in arrs])
        ns = np.asarray([len(v) for v in arrs] if lens is None else lens, np.int32)
        return lib.bark_hip_resample_many(h, ptrs, ns.ctypes.data, len(arrs), a, C.byref(to), out.ctypes.data, cap, n_out.ctypes.data)

    assert one(x, 0) == -1 and one(x, -3) == -1 and one(None, 10) == -1
    big = np.zeros(ofr.MAX_SAMPLES + 1, np.float32)
    assert one(big, len(big), 24000, 8000) == -1
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[1234] = bad
        assert one(y, len(y)) == -1 and many([x, y], pkg.audio_format(8000, "mulaw")) == -1, bad
    assert one(x, len(x), 11025, 24000) == -1 and one(x, len(x), 24000, 11025) == -1 and one(x, len(x), 16000, 48000) == -1 and one(x, len(x), 16000, 16000) == -1
    assert one(x, len(x), cap=1999) == -1 and one(x, len(x), cap=2000) == 2000               # capacity in floats
    s16 = pkg.audio_format(48000, "s16")
    assert many([x], s16, cap=11999) == -1 and many([x], s16, cap=12000) == 12000 and int(n_out[0]) == 6000      # one byte short
    assert many([x, x], pkg.audio_format(8000, "mulaw"), cap=1999) == -1 and many([x, x], pkg.audio_format(8000, "mulaw"), cap=2000) == 2000
    assert many([x], pkg.audio_format(48000, 3)) == -1 and many([x], pkg.audio_format(48000, -1)) == -1 and many([x], pkg.audio_format(11025, 0)) == -1
    assert many([x] * 65, s16) == -1 and many([x, x], s16, lens=[3000, 0]) == -1
    assert lib.bark_hip_resample(None, x.ctypes.data, 10, 24000, 16000, out.ctypes.data, 100) == -1
    with pytest.raises(ValueError):
        ctx.resample(x, 11025, 24000)
    with pytest.raises(ValueError):
        ctx.resample(x[:0], 24000, 16000)
    _same("after the refusals", ctx.resample(x, 24000, 16000), good)
    assert ctx.generate_audio(TEXT) and len(ctx.audio_data()) > 0                            # the context still generates


def test_old_kernel_and_new_kernel_agree_at_24000_to_16000(ctx):
    for n in (1, 23, 767, 768, 1537, 20011):
        x = rr.dense_signal(n, seed=n)
        old = ctx.resample_24k_to_16k(x)
        _same(f"C13r kernel against its rule, n={n}", old, rr.resample(x))
        _same(f"C14r kernel against the C13r kernel, n={n}", ctx.resample(x, 24000, 16000), old)
    assert ctx.time_resample_pair(24000, 24000, 44100, "mulaw", 3) > 0.0 and ctx.time_resample(24000, 3) > 0.0


# ---- O5: the routes that convert a generation -------------------------------------------------------------------------------------------------------------
ROUTE_FORMATS = [(8000, "mulaw"), (48000, "s16"), (44100, "f32"), (24000, "s16"), (24000, "f32")]


def test_get_audio_as_and_batch_audio_as_are_resample_many_of_the_result(ctx):
    assert ctx.generate_audio(TEXT)
    pcm = np.asarray(ctx.audio_data(), np.float32).copy()
    for rate, name in ROUTE_FORMATS:
        _same(f"get_audio_as {rate} {name}", ctx.audio_as(rate, name), ctx.resample_many([pcm], 24000, rate, fmt=name)[0])
    assert ctx.audio_as(24000, "f32").tobytes() == pcm.tobytes() and np.asarray(ctx.audio_data(), np.float32).tobytes() == pcm.tobytes()
    to = _pkg().audio_format(16000, "s16")
    n16 = ofr.n_out(len(pcm), 24000, 16000)
    buf = np.zeros(2 * n16, np.uint8)
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(to), buf.ctypes.data, 2 * n16 - 1) == -2 - 2 * n16                # too small: -(2 + bytes)
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(to), buf.ctypes.data, 2 * n16) == 2 * n16
    bad = _pkg().audio_format(11025, "s16")
    assert ctx._lib.bark_hip_get_audio_as(ctx._h, C.byref(bad), buf.ctypes.data, buf.size) == -1
    res = ctx.generate_batch([TEXT, "another one", "third"])
    assert all(r is not None for r in res)
    for i, r in enumerate(res):
        for rate, name in ROUTE_FORMATS[:3]:
            _same(f"batch_audio_as {i} {rate} {name}", ctx.batch_audio_as(i, rate, name), ctx.resample_many([r["pcm"]], 24000, rate, fmt=name)[0])
    assert ctx._lib.bark_hip_batch_audio_as(ctx._h, 3, C.byref(to), buf.ctypes.data, buf.size) == -1
    fresh = _load()
    try:
        assert fresh._lib.bark_hip_get_audio_as(fresh._h, C.byref(to), buf.ctypes.data, buf.size) == -1                      # no audio held
    finally:
        fresh.free()


@pytest.mark.concurrency
def test_collector_job_with_three_formats(ctx):
    pkg = _pkg()
    texts = [TEXT, "another one", "third", "and a fourth", "five"]
    fmts = [pkg.audio_format(8000, "mulaw"), None, pkg.audio_format(48000, "s16"), pkg.audio_format(8000, "mulaw"), pkg.audio_format(48000, "s16")]
    owner = _load(temp=0.7, fine_temp=0.5)
    try:
        with pkg.Batcher(owner, max_batch=8, max_wait_ms=200) as b:
            tickets = [b.submit(t, seed=40 + i, audio_format=f) for i, (t, f) in enumerate(zip(texts, fmts))]
            plain = [b.submit(t, seed=40 + i) for i, t in enumerate(texts)]                  # the same requests in the engine's own format
            probe = np.zeros(4, np.float32)
            assert b._lib.bark_hip_batcher_wait(b._b, tickets[0], probe.ctypes.data, 4) == -1             # not f32: refused, the ticket stays valid
            got = [b.wait_bytes(t) for t in tickets]
            ref = [b.wait(t) for t in plain]
            bad = pkg.audio_format(11025, "s16")
            assert b._lib.bark_hip_batcher_submit_as(b._b, b"x", None, None, None, C.byref(bad)) == -1
    finally:
        owner.free()
    for i, (g, f, r) in enumerate(zip(got, fmts, ref)):
        assert len(r) > 0
        if f is None:
            assert g.dtype == np.float32 and g.tobytes() == r.tobytes()                      # the default request: the bytes of bark_hip_batcher_wait
        else:
            name = {0: "f32", 1: "s16", 2: "mulaw"}[f.sample_format]
            _same(f"request {i} {f.sample_rate} {name}", g, ctx.resample_many([r], 24000, f.sample_rate, fmt=name)[0])


# ---- O6: the server ---------------------------------------------------------------------------------------------------------------------------------------
def _chunks(wav):
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE" and struct.unpack_from("<I", wav, 4)[0] == len(wav) - 8
    out, pos = {}, 12
    while pos + 8 <= len(wav):
        size = struct.unpack_from("<I", wav, pos + 4)[0]
        out[wav[pos:pos + 4]] = wav[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    return out


@pytest.mark.concurrency
def test_native_batch_server_formats_and_resampled_recordings(tmp_path):
    from test_gpu_voice_from_audio import _Server, _hubert, _wav16
    pkg = _pkg()
    i16 = np.round(cref.fixture_signal(16000).astype(np.float64) * 20000.0).astype(np.int16)                # one second "at 16 kHz"
    rec = i16.astype(np.float32) / np.float32(32768.0)
    with _Server("-m", _model("toy_enc"), "--semantic-encoder", _hubert("hub_toy")) as srv:
        st, mu = srv.request("POST", "/bark", json.dumps({"text": TEXT, "sample_rate": 8000, "format": "mulaw"}).encode())
        assert st == 200
        st, s16 = srv.request("POST", "/bark", json.dumps({"text": TEXT, "sample_rate": 48000, "format": "s16"}).encode())
        assert st == 200
        st, plain = srv.request("POST", "/bark", json.dumps({"text": TEXT}).encode())
        assert st == 200
        for body in ({"text": TEXT, "sample_rate": 11025}, {"text": TEXT, "format": "alaw"}, {"text": TEXT, "format": 1}, {"text": TEXT, "sample_rate": "x"}):
            assert srv.request("POST", "/bark", json.dumps(body).encode())[0] == 400, body
        assert srv.request("POST", "/voices?name=r", _wav16(i16, rate=16000))[0] == 400                      # without the switch: as before
        assert srv.request("POST", "/voices?name=r&resample=1", _wav16(i16, rate=11025))[0] == 400          # not a rate of the list
        st, body = srv.request("POST", "/voices?name=r&resample=1", _wav16(i16, rate=16000))
        assert st == 200 and json.loads(body)["name"] == "r", (st, body)
        st, voice_bytes = srv.request("GET", "/voices/r")
        assert st == 200
    pcm = np.frombuffer(plain[44:], np.float32)
    one = _load("toy_enc", n_steps_text_encoder=768)
    try:
        one.set_fine_order(2)
        assert one.generate_audio(TEXT)
        assert np.asarray(one.audio_data(), np.float32).tobytes() == pcm.tobytes()
        want_mu = one.resample_many([pcm], 24000, 8000, fmt="mulaw")[0]
        want_s16 = one.resample_many([pcm], 24000, 48000, fmt="s16")[0]
        one.load_semantic_encoder(_hubert("hub_toy"))
        v = pkg.VoicePrompt(*one.voice_from_audio(one.resample(rec, 16000, 24000)))
        assert pkg.voice.from_audio_native(one, rec, rate=16000) == v
    finally:
        one.free()
    ch = _chunks(mu)
    assert struct.unpack("<HHIIHHH", ch[b"fmt "]) == (7, 1, 8000, 8000, 1, 8, 0) and struct.unpack("<I", ch[b"fact"]) == (len(want_mu),)
    assert ch[b"data"] == want_mu.tobytes()
    ch = _chunks(s16)
    assert struct.unpack("<HHIIHH", ch[b"fmt "]) == (1, 1, 48000, 96000, 2, 16) and ch[b"data"] == want_s16.tobytes() and b"fact" not in ch
    ch = _chunks(plain)
    assert struct.unpack("<HHIIHH", ch[b"fmt "]) == (3, 1, 24000, 96000, 4, 32)
    path = str(tmp_path / "r.bvp")
    v.save(path)
    assert voice_bytes == open(path, "rb").read()
    # the defaults come from the flags
    with _Server("-m", _model("toy_enc"), "--sample-rate", "8000", "--format", "mulaw") as srv:
        st, mu2 = srv.request("POST", "/bark", json.dumps({"text": TEXT}).encode())
        assert st == 200 and mu2 == mu
