"""GPU tests of voice prompts from a recording in the C API and the batch server: the device resampler (rule C13r: bark_hip_resample_24k_to_16k) bit for bit
against tests/resample_ref.py, the composition bark_hip_voice_from_audio / bark_hip_set_voice_from_audio against the calls it is made of, their refusals, and
bark_batch_server's POST /voices.  Everything here is an equality of bits: the resampler against its restatement, the composition against its parts."""
import json
import os
import socket
import struct
import subprocess
import threading
import time
import urllib.error
import urllib.request

import numpy as np
import pytest

import codec_encoder_ref as cref
import resample_ref as rr

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_IN = 768                   # input samples of one workgroup of resample_24k_16k_kernel as built (512 outputs)
MAX_USED = 480000               # BARK_HIP_VOICE_AUDIO_MAX_SAMPLES
SHORTEST = 1079                 # the shortest recording that leaves a history: 720 samples at 16 kHz = 2 semantic ids, 4 codec frames
TEXT = "hello world this is bark"


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


def _hubert(preset):
    from tools.make_synth_hubert import ensure_hubert
    return ensure_hubert(preset, 0)


def _load(bark_preset, hub_preset, **over):
    pkg = _pkg()
    par = dict(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32)
    par.update(over)
    ctx = pkg.BarkContext.load_model(_model(bark_preset), pkg.default_params(**par), seed=0)
    if hub_preset:
        ctx.load_semantic_encoder(_hubert(hub_preset))
    return ctx


class _Env:
    """contexts made on first use and shared by the tests of the module: "toy" = toy_enc + hub_toy, "small" = small + hub_base"""

    def __init__(self):
        self.ctxs = {}

    def ctx(self, which):
        if which not in self.ctxs:
            self.ctxs[which] = _load("toy_enc", "hub_toy") if which == "toy" else _load("small", "hub_base")
        return self.ctxs[which]

    def close(self):
        for c in self.ctxs.values():
            c.free()


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


def _signal(kind, n):
    if kind == "fixture":
        return cref.fixture_signal(n) if n <= 24000 else rr.dense_signal(n)
    return np.random.default_rng([17, n]).standard_normal(n).astype(np.float32)


def _same_bits(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:5]]} != {want.reshape(-1)[bad[:5]]}"


# ---- V1: the resampler against C13r -------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 4, 21, 22, 23, TILE_IN - 1, TILE_IN, TILE_IN + 1, 2 * TILE_IN - 1, 2 * TILE_IN, 2 * TILE_IN + 1, 24000]


@pytest.mark.parametrize("kind", ["fixture", "random"])
@pytest.mark.parametrize("n", LENGTHS, ids=lambda v: f"n{v}-")
def test_resampler_is_c13r_bit_for_bit(env, n, kind):
    x = _signal(kind, n)
    got = env.ctx("toy").resample_24k_to_16k(x)
    assert len(got) == (2 * n + 2) // 3
    _same_bits(f"resampler n={n} {kind}", got, rr.resample(x))


@pytest.mark.parametrize("n", [23, 2 * TILE_IN + 1], ids=lambda v: f"n{v}-")
def test_resampler_unit_impulses_read_the_taps_back_through_the_edges(env, n):
    ctx = env.ctx("toy")
    h = rr.taps()
    for pos in list(range(12)) + list(range(n - 12, n)):
        x = np.zeros(n, np.float32); x[pos] = 1.0
        got = ctx.resample_24k_to_16k(x)
        _same_bits(f"impulse at {pos} of {n}", got, rr.resample(x))
        m = np.arange(len(got))
        j = pos - (3 * m) // 2
        inside = (j >= -10) & (j <= 11)
        want = np.where(inside, h[m & 1, np.clip(j + 10, 0, 21)], np.float32(0.0)).astype(np.float32)
        assert np.array_equal(got, want), pos


def test_resampler_at_the_longest_recording(env):
    n = rr.MAX_SAMPLES
    x = rr.dense_signal(n)
    got = env.ctx("toy").resample_24k_to_16k(x)
    n_out = rr.n_out(n)
    assert len(got) == n_out
    m = np.unique(np.concatenate([np.arange(4096), np.arange(n_out - 4096, n_out), np.random.default_rng(23).integers(4096, n_out - 4096, 4096)]))
    _same_bits("resampler at 1 310 720 samples", got[m], rr.resample(x, m))
    assert np.count_nonzero(got) > n_out - 100


def test_resampler_twice_and_on_a_clone(env):
    ctx = env.ctx("toy")
    long, short = _signal("fixture", 24000), _signal("random", 2 * TILE_IN + 1)
    first = ctx.resample_24k_to_16k(long)
    _same_bits("second call", ctx.resample_24k_to_16k(long), first)
    after_long = ctx.resample_24k_to_16k(short)          # the buffers hold the long call's samples behind the short one's
    _same_bits("short after long", after_long, rr.resample(short))
    cl = ctx.clone(seed=1)
    try:
        _same_bits("clone", cl.resample_24k_to_16k(long), first)
        _same_bits("clone, short", cl.resample_24k_to_16k(short), after_long)
    finally:
        cl.free()
    bare = _load("toy", None)                             # neither encoder: the resampler needs none
    try:
        assert not bare.has_semantic_encoder() and not bare.has_codec_encoder()
        _same_bits("no encoders", bare.resample_24k_to_16k(long), first)
        assert bare.time_resample(24000, 3) > 0.0
    finally:
        bare.free()


# ---- V2: the composition ------------------------------------------------------------------------------------------------------------------------------
def _parts(ctx, pcm):
    """what bark_hip_voice_from_audio is made of, call by call (the resampler is the device one)"""
    sem = ctx.semantic_encode(ctx.resample_24k_to_16k(pcm))
    codes = ctx.codec_encode(pcm, 8)
    return sem, np.ascontiguousarray(codes[:2].T), np.ascontiguousarray(codes.T)


COMPOSITION = [("toy", SHORTEST), ("toy", 24000), ("small", 24000)]


@pytest.mark.parametrize("which,n", COMPOSITION, ids=[f"{w}-n{n}-" for w, n in COMPOSITION])
def test_voice_from_audio_equals_its_parts(env, which, n):
    pkg = _pkg()
    ctx = env.ctx(which)
    pcm = cref.fixture_signal(n)
    sem, coarse, fine = ctx.voice_from_audio(pcm)
    want = _parts(ctx, pcm)
    _same_bits("semantic", sem, want[0]); _same_bits("coarse", coarse, want[1]); _same_bits("fine", fine, want[2])
    assert len(sem) == ((2 * n + 2) // 3 - 400) // 320 + 1 and fine.shape == ((n + 319) // 320, 8) and np.array_equal(coarse, fine[:, :2])
    v = pkg.voice.from_audio_native(ctx, pcm)
    assert v == pkg.VoicePrompt(*want)
    ctx.set_voice_prompt(v)                               # what the call returns has passed the checks of bark_hip_set_voice_prompt
    ctx.set_voice_prompt(None)


@pytest.mark.parametrize("n", [MAX_USED + 1, 700000], ids=lambda v: f"n{v}-")
def test_long_recordings_are_used_from_their_last_480000_samples(env, n):
    ctx = env.ctx("toy")
    pcm = rr.dense_signal(n)
    got = ctx.voice_from_audio(pcm)
    want = ctx.voice_from_audio(pcm[n - MAX_USED:])
    for name, g, w in zip(("semantic", "coarse", "fine"), got, want):
        _same_bits(name, g, w)
    assert len(got[0]) == 999 and len(got[2]) == 1500
    if n == 700000:                                       # ... and the last 480 000 samples through the parts
        for name, g, w in zip(("semantic", "coarse", "fine"), got, _parts(ctx, pcm[n - MAX_USED:])):
            _same_bits(name + " (parts)", g, w)


# ---- V3: set_voice_from_audio and generation ----------------------------------------------------------------------------------------------------------
def _generate(ctx):
    assert ctx.generate_audio(TEXT)
    return [ctx.semantic_tokens().copy(), ctx.coarse_tokens().copy(), ctx.fine_tokens().copy(), np.asarray(ctx.audio_data(), np.float32).copy()]


def test_set_voice_from_audio_is_set_voice_prompt_with_the_same_arrays(env):
    pkg = _pkg()
    ctx = env.ctx("toy")
    pcm = cref.fixture_signal(24000)
    fresh = _load("toy_enc", None)                        # never sees a new call
    try:
        plain = _generate(fresh)
    finally:
        fresh.free()
    try:
        ctx.set_voice_from_audio(pcm)
        a = _generate(ctx)
        ctx.set_voice_prompt(None)
        ctx.set_voice_prompt(pkg.VoicePrompt(*ctx.voice_from_audio(pcm)))
        b = _generate(ctx)
        for name, x, y in zip(("semantic", "coarse", "fine", "pcm"), a, b):
            _same_bits(name, x, y)
        assert len(a[3]) == 320 * len(a[2]) > 0
        assert not all(np.array_equal(x, y) for x, y in zip(a, plain))         # the voice steers the generation
    finally:
        ctx.set_voice_prompt(None)
    for name, x, y in zip(("semantic", "coarse", "fine", "pcm"), _generate(ctx), plain):
        _same_bits("without a voice: " + name, x, y)


# ---- V4: refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(env):
    pkg = _pkg()
    ctx = env.ctx("toy")
    lib, h = ctx._lib, ctx._h
    x = cref.fixture_signal(24000)
    good_rs = ctx.resample_24k_to_16k(x)
    good_v = ctx.voice_from_audio(x)
    out = np.zeros(rr.n_out(rr.MAX_SAMPLES) + 8, np.float32)
    sem, coarse, fine = np.zeros(1024, np.int32), np.zeros((1500, 2), np.int32), np.zeros((1500, 8), np.int32)
    ns, nf = np.zeros(1, np.int32), np.zeros(1, np.int32)

    def rs(arr, n, cap=out.size, c=None):
        return lib.bark_hip_resample_24k_to_16k((c or ctx)._h, None if arr is None else arr.ctypes.data, n, out.ctypes.data, cap)

    def vfa(arr, n, sem_cap=sem.size, rows=1500, c=None):
        return lib.bark_hip_voice_from_audio((c or ctx)._h, arr.ctypes.data, n, sem.ctypes.data, sem_cap, coarse.ctypes.data, fine.ctypes.data, rows, ns.ctypes.data, nf.ctypes.data)

    def setv(arr, n, c=None):
        return lib.bark_hip_set_voice_from_audio((c or ctx)._h, arr.ctypes.data, n)

    def still_good():
        _same_bits("resampler after a refusal", ctx.resample_24k_to_16k(x), good_rs)
        for g, w in zip(ctx.voice_from_audio(x), good_v):
            _same_bits("voice after a refusal", g, w)

    # the resampler
    big = np.zeros(rr.MAX_SAMPLES + 1, np.float32)
    assert rs(x, 0) == -1 and rs(x, -5) == -1 and rs(big, len(big)) == -1 and rs(None, 10) == -1
    assert rs(big, rr.MAX_SAMPLES) == rr.n_out(rr.MAX_SAMPLES)                              # the longest one that is taken
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[777] = bad
        assert rs(y, len(y)) == -1, bad
    y = x.copy(); y[777] = 65520.0
    assert rs(y, len(y)) == 16000                                                           # finite: the resampler itself knows no f16
    assert rs(x, len(x), 15999) == -1 and rs(x, len(x), 16000) == 16000                     # capacity
    assert lib.bark_hip_resample_24k_to_16k(None, x.ctypes.data, 10, out.ctypes.data, out.size) == -1
    still_good()
    # the composition: length, samples, capacities
    assert vfa(x, 598) == -1 and vfa(x, 0) == -1 and vfa(x, -1) == -1 and setv(x, 598) == -1
    for n in (599, SHORTEST - 1):                                                           # one semantic id: no history is left
        assert vfa(x, n) == -1 and setv(x, n) == -1, n
    assert vfa(x, SHORTEST) == 0 and (int(ns[0]), int(nf[0])) == (2, 4)
    for bad in (np.nan, np.inf, 65520.0, -1e5):
        y = x.copy(); y[20000] = bad
        assert vfa(y, len(y)) == -1 and setv(y, len(y)) == -1, bad
    assert vfa(x, len(x), sem_cap=48) == -1 and vfa(x, len(x), rows=74) == -1
    assert vfa(x, len(x), sem_cap=49, rows=75) == 0 and (int(ns[0]), int(nf[0])) == (49, 75)
    still_good()
    # a token head whose ids lie outside the model's semantic vocabulary
    ctx.set_params(pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32, semantic_vocab_size=1))
    try:
        assert good_v[0].max() >= 1
        assert vfa(x, len(x)) == -1 and setv(x, len(x)) == -1
    finally:
        ctx.set_params(pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32))
    still_good()
    # a refused set call keeps the voice the context had
    ctx.set_voice_from_audio(x)
    try:
        kept = ctx.tokenize("x")
        assert setv(x, 598) == -1
        assert np.array_equal(ctx.tokenize("x"), kept) and not np.array_equal(kept[256:512], np.full(256, 10000))
    finally:
        ctx.set_voice_prompt(None)
    # no semantic encoder; no codec encoder in the file
    for bark_preset, hub_preset in (("toy_enc", None), ("toy", "hub_toy")):
        c = _load(bark_preset, hub_preset)
        try:
            assert vfa(x, len(x), c=c) == -1 and setv(x, len(x), c=c) == -1
            assert rs(x, len(x), c=c) == 16000 and np.array_equal(out[:16000].view(np.uint32), good_rs.view(np.uint32))
            assert c.generate_audio("hello")
        finally:
            c.free()
    with pytest.raises(ValueError):
        ctx.voice_from_audio(x[:598])
    with pytest.raises(ValueError):
        pkg.voice.from_audio_native(ctx, x[:598])
    still_good()


# ---- V5: the server -----------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _wav16(samples_i16, rate=24000, channels=1):
    data = np.asarray(samples_i16, "<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * channels * 2, channels * 2, 16)
    body = b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


class _Server:
    """bark_batch_server as a child that is killed when the block ends, or after 240 s whatever happens"""

    def __init__(self, *args):
        self.port = _free_port()
        exe = os.path.join(ROOT, "bark.cpp_amd", "lib", "bark_batch_server")
        self.proc = subprocess.Popen([exe, "-p", str(self.port), "--temp", "0", "--fine-temp", "0", "--max-wait-ms", "10", *args],
                                     stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        self.limit = threading.Timer(240.0, self.proc.kill)
        self.limit.daemon = True
        self.limit.start()

    def __enter__(self):
        for _ in range(600):
            try:
                urllib.request.urlopen(f"http://127.0.0.1:{self.port}/", timeout=2).read()
                return self
            except Exception:
                if self.proc.poll() is not None:
                    raise AssertionError(self.proc.stderr.read().decode()[-1500:])
                time.sleep(0.1)
        self.__exit__(None, None, None)
        raise AssertionError("the server did not start")

    def __exit__(self, *exc):
        self.limit.cancel()
        self.proc.kill(); self.proc.wait()

    def request(self, method, path, data=None):
        """(status, body)"""
        req = urllib.request.Request(f"http://127.0.0.1:{self.port}{path}", data=data, method=method)
        try:
            with urllib.request.urlopen(req, timeout=200) as r:
                return r.status, r.read()
        except urllib.error.HTTPError as e:
            return e.code, e.read()

    def status_for_announced_length(self, path, length):
        """the status line for a POST that announces `length` bytes and sends none of them"""
        with socket.create_connection(("127.0.0.1", self.port), timeout=30) as s:
            s.sendall(f"POST {path} HTTP/1.1\r\nHost: x\r\nContent-Length: {length}\r\n\r\n".encode())
            head = b""
            while b"\r\n" not in head:
                k = s.recv(4096)
                if not k:
                    break
                head += k
        return int(head.split()[1])


@pytest.mark.concurrency
def test_native_batch_server_voice_from_a_recording(env, tmp_path):
    pkg = _pkg()
    i16 = np.round(cref.fixture_signal(24000).astype(np.float64) * 20000.0).astype(np.int16)
    pcm = i16.astype(np.float32) / np.float32(32768.0)                     # what the server decodes
    ctx = env.ctx("toy")
    v = pkg.voice.from_audio_native(ctx, pcm)
    path = str(tmp_path / "a.bvp")
    v.save(path)
    at_start = tmp_path / "start.wav"
    at_start.write_bytes(_wav16(i16))
    with _Server("-m", _model("toy_enc"), "--semantic-encoder", _hubert("hub_toy"), "--voice-audio", f"0start={at_start}") as srv:
        assert srv.request("GET", "/voices") == (200, b'{"voices": ["0start"]}')
        assert srv.request("GET", "/voices/0start") == (200, open(path, "rb").read())
        st, body = srv.request("POST", "/voices?name=a", _wav16(i16))
        assert st == 200 and json.loads(body) == {"name": "a", "n_semantic": 49, "n_frames": 75}, (st, body)
        st, body = srv.request("GET", "/voices/a")
        assert st == 200 and body == open(path, "rb").read()
        assert srv.request("GET", "/voices") == (200, b'{"voices": ["0start", "a"]}')
        assert srv.request("GET", "/voices/b")[0] == 404
        # refusals
        assert srv.request("POST", "/voices?name=s", _wav16(np.repeat(i16, 2), channels=2))[0] == 400          # stereo
        assert srv.request("POST", "/voices?name=r", _wav16(i16, rate=16000))[0] == 400                          # 16 kHz
        assert srv.request("POST", "/voices?name=bad/name", _wav16(i16))[0] == 400 and srv.request("POST", "/voices", _wav16(i16))[0] == 400
        assert srv.request("POST", "/voices?name=t", _wav16(i16)[:-10])[0] == 400                                 # a data chunk beyond the body
        assert srv.request("POST", "/voices?name=q", _wav16(i16[:500]))[0] == 400                                 # too short for the engine
        assert srv.status_for_announced_length("/voices?name=big", (4 << 20) + 1) == 413
        assert srv.status_for_announced_length("/bark", (1 << 20) + 1) == 413                                      # /bark keeps its own limit
        assert srv.request("GET", "/voices") == (200, b'{"voices": ["0start", "a"]}')
        # a request in that voice: what a single context with the voice generates (the fine order of the server's jobs, the server's 768 steps)
        st, wav = srv.request("POST", "/bark", json.dumps({"text": TEXT, "voice": "a"}).encode())
        assert st == 200
        st, wav_plain = srv.request("POST", "/bark", json.dumps({"text": TEXT}).encode())
        assert st == 200
        assert srv.request("POST", "/bark", json.dumps({"text": TEXT, "voice": "nobody"}).encode())[0] == 400
    one = _load("toy_enc", None, n_steps_text_encoder=768)
    try:
        one.set_fine_order(2)
        assert one.generate_audio(TEXT)
        plain = np.asarray(one.audio_data(), np.float32).copy()
        one.set_voice_prompt(v)
        assert one.generate_audio(TEXT)
        voiced = np.asarray(one.audio_data(), np.float32).copy()
    finally:
        one.free()
    assert wav[:4] == b"RIFF" and wav_plain[:4] == b"RIFF"
    _same_bits("voiced pcm from the server", np.frombuffer(wav[44:], np.float32), voiced)
    _same_bits("a request without the field has no voice", np.frombuffer(wav_plain[44:], np.float32), plain)
    assert not np.array_equal(voiced, plain)
    # no semantic encoder: the route answers 409
    with _Server("-m", _model("toy_enc")) as srv:
        assert srv.request("POST", "/voices?name=a", _wav16(i16))[0] == 409
        assert srv.request("GET", "/voices") == (200, b'{"voices": []}')
