"""GPU tests of long-form text (rules C15s and C15j): the join kernels bit for bit against tests/long_form_ref.py with the library's
own tap tables - all rates and formats, runs of one-sample segments, tiles inside a gap and across several seams, trim, fade, the old resampler beside the
new kernel, repeats, clones and refusals - and bark_hip_generate_long on the toy model: the spans against the splitter's rule, every chunk against a job of
that chunk alone, the joined audio against the rule, chained voices.  Everything here is an equality of bits or bytes."""
import ctypes as C

import numpy as np
import pytest

import long_form_ref as lfr
import output_format_ref as ofr
import resample_ref as rr

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

FMT = {"f32": ofr.F32, "s16": ofr.S16, "mulaw": ofr.MULAW}
OUTPUTS = [(r, "f32") for r in ofr.RATES] + [(8000, "s16"), (8000, "mulaw"), (44100, "s16"), (44100, "mulaw")]
LENGTHS = (1, 2, 239, 240, 241, 1, 1, 1, 5000, 1025)
LONG_TEXT = "hello world. this is bark speech, a model of audio and water and the river! go there? yes"


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _load(**over):
    from tools.make_synth_model import ensure_model
    pkg = _pkg()
    par = dict(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32)
    par.update(over)
    return pkg.BarkContext.load_model(ensure_model("toy", 0), pkg.default_params(**par), seed=0)


@pytest.fixture(scope="module")
def ctx():
    c = _load()
    yield c
    c.free()


@pytest.fixture(scope="module")
def tables():
    """the library's own table of every pair from 24000, [L][2 HALF]"""
    lib = _pkg().load_library()
    out = {}
    for rate in ofr.RATES:
        if rate == 24000:
            continue
        lmh = np.zeros(3, np.int32)
        n = lib.bark_hip_resample_table(24000, rate, None, 0, lmh.ctypes.data)
        h = np.zeros(n, np.float32)
        assert n > 0 and lib.bark_hip_resample_table(24000, rate, h.ctypes.data, n, lmh.ctypes.data) == n
        out[rate] = h.reshape(int(lmh[0]), 2 * int(lmh[2]))
    return out


def _jp(**p):
    return _pkg().join_params(**p)


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: {got.reshape(-1)[bad[:5]]} != {want.reshape(-1)[bad[:5]]}"


def _check(ctx, tables, what, segs, p, rate, name="f32"):
    """one join against the rule: the bytes and the layout"""
    got, lay = ctx.join_many(segs, _jp(**p), rate, name, want_layout=True)
    _same(f"{what} {rate} {name} {p}", got, lfr.joined(segs, p, rate, FMT[name], h=tables.get(rate)))
    assert lay == lfr.layout(segs, p)[0], (what, p)
    return got


def _segments(lengths, seed=0):
    return [rr.dense_signal(n, seed=seed + 31 * k + n) for k, n in enumerate(lengths)]


# ---- J1: the join against the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,name", OUTPUTS, ids=[f"{r}-{n}" for r, n in OUTPUTS])
def test_join_is_c15j_bit_for_bit(ctx, tables, rate, name):
    segs = _segments(LENGTHS)
    for gap in (0, 1, 7, 6000):
        _check(ctx, tables, "join", segs, dict(gap_samples=gap), rate, name)
    _check(ctx, tables, "join, trimmed and faded", segs, dict(gap_samples=7, fade_samples=240, trim_threshold=0.05, trim_pad_frames=1), rate, name)


# ---- J2: runs of one-sample segments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 48000])
def test_runs_of_one_sample_segments(ctx, tables, rate):
    """at 8000 Hz HALF = 20: the 40 taps of one output reach over up to 40 segments"""
    assert ofr.lmh(24000, 8000)[2] == 20
    segs = [np.array([v], np.float32) for v in rr.dense_signal(40, seed=2)]
    for gap in (0, 1):
        _check(ctx, tables, "one-sample segments", segs, dict(gap_samples=gap), rate)
        _check(ctx, tables, "one-sample segments, faded", segs, dict(gap_samples=gap, fade_samples=1), rate)


# ---- J3: tiles ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_tile_inside_a_gap_and_a_tile_with_many_seams(ctx, tables):
    # 8000 Hz: a tile of 1024 outputs reads 3072 samples of J; outputs 1024 .. 3023 lie in the gap behind the first segment, so tile 1 sees no sample at all
    segs = _segments((3072, 500, 3))
    got = _check(ctx, tables, "tile in a gap", segs, dict(gap_samples=6000), 8000)
    assert len(got) == -(-(3072 + 6000 + 500 + 6000 + 3) // 3) and np.all(got[1100:1900] == 0.0) and np.any(got[:1024] != 0.0)
    # twelve segments of 200 .. 300 samples with gaps of 7: every tile of every rate holds three seams or more
    segs = _segments([200 + 9 * k for k in range(12)], seed=5)
    for rate in (8000, 24000, 44100, 48000):
        _check(ctx, tables, "seams", segs, dict(gap_samples=7, fade_samples=16), rate)


@pytest.mark.parametrize("n_out", [1023, 1024, 1025])
def test_output_counts_around_one_tile(ctx, tables, n_out):
    for rate, N in ((24000, n_out), (8000, 3 * n_out - 2), (8000, 3 * n_out)):
        segs = _segments((N - 700 - 5, 700))
        got = _check(ctx, tables, "tile edge", segs, dict(gap_samples=5), rate, "s16")
        assert len(got) == n_out


# ---- J4: trim ----------------------------------------------------------------------------------------------------------------------------------------------
def _lone(n, at, v=0.5):
    x = np.full(n, 0.01, np.float32)
    x[at] = v
    return x


def test_trim_by_frame_activity(ctx, tables):
    n = 1000
    cases = [[_lone(n, 0)], [_lone(n, 239)], [_lone(n, 240)], [_lone(n, n - 1)], [_lone(241, 240)], [_lone(241, 3)], [_lone(n, 500, -0.5)], [_lone(n, 500, -0.75)],
             [_lone(n, 0), _lone(n, n - 1), _lone(241, 240)]]
    for k, segs in enumerate(cases):
        for pad in (0, 1, 3):
            for rate in (24000, 8000):
                _check(ctx, tables, f"trim case {k}", segs, dict(gap_samples=11, trim_threshold=0.5, trim_pad_frames=pad), rate)
    # a threshold equal to the peak counts as active, the next float above it does not
    x = _lone(n, 500, 0.5)
    lay = ctx.join_many([x], _jp(trim_threshold=0.5), want_layout=True)[1]
    assert lay == [(0, 240)]
    got, lay = ctx.join_many([x], _jp(trim_threshold=float(np.nextafter(np.float32(0.5), np.float32(1.0)))), want_layout=True)
    assert lay == [(0, 0)] and len(got) == 0


def test_silent_segments_take_no_gap(ctx, tables):
    loud, quiet = rr.dense_signal(700, seed=1), np.full(500, 0.001, np.float32)
    loud[3] = 0.9
    p = dict(gap_samples=100, trim_threshold=0.02, trim_pad_frames=0)
    for order in ([quiet, loud, loud], [loud, quiet, loud], [loud, loud, quiet], [quiet, quiet, loud, quiet, loud, quiet]):
        for rate in (24000, 16000):
            _check(ctx, tables, "silent segment", order, p, rate)
    a = lfr.layout([loud, quiet, loud], p)
    b = lfr.layout([loud, loud], p)
    assert a[1] == b[1]                                                                      # the same length: no gap was doubled
    for rate, name in ((24000, "f32"), (8000, "mulaw")):
        got, lay = ctx.join_many([quiet, quiet], _jp(**p), rate, name, want_layout=True)
        assert len(got) == 0 and lay == [(0, 0), (0, 0)]                                     # all silent: no bytes


# ---- J5: fade ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 240])
def test_fade_at_every_length_around_2f(ctx, tables, F):
    segs = [np.ones(K, np.float32) * np.float32(0.75) for K in (1, 2, 2 * F - 1, 2 * F, 2 * F + 1)] + _segments((2 * F + 1, 1, 2))
    for rate in (24000, 12000):
        _check(ctx, tables, "fade", segs, dict(gap_samples=3, fade_samples=F), rate)
    J = ctx.join_many(segs[:5], _jp(gap_samples=0, fade_samples=F))
    _same("the fade table itself", J[-(2 * F + 1):][:F], (np.float32(0.75) * lfr.fade_table(F)).astype(np.float32))


# ---- J6: the old kernel beside the new one ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", ofr.RATES)
def test_one_plain_segment_equals_resample_many(ctx, rate):
    x = rr.dense_signal(5003, seed=6)
    for name in FMT:
        _same(f"{rate} {name}", ctx.join_many([x], _jp(gap_samples=0), rate, name), ctx.resample_many([x], 24000, rate, fmt=name)[0])


# ---- J7: repeats and clones ------------------------------------------------------------------------------------------------------------------------------------
def test_repeat_and_clone_give_the_same_bytes(ctx):
    segs = _segments(LENGTHS, seed=9)
    p = _jp(gap_samples=50, fade_samples=32, trim_threshold=0.05, trim_pad_frames=1)
    first = ctx.join_many(segs, p, 44100, "s16")
    assert ctx.join_many(segs, p, 8000, "mulaw").dtype == np.uint8                           # another format and fade in between
    assert ctx.join_many(segs, _jp(fade_samples=7), 44100, "s16").tobytes() != first.tobytes()
    assert ctx.join_many(segs, p, 44100, "s16").tobytes() == first.tobytes()
    twin = ctx.clone(seed=1)
    try:
        assert twin.join_many(segs, p, 44100, "s16").tobytes() == first.tobytes()
    finally:
        twin.free()


# ---- J8: refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx, tables):
    pkg = _pkg()
    lib, h = ctx._lib, ctx._h
    x = rr.dense_signal(3000)
    out = np.zeros(1 << 16, np.uint8)
    lay = np.zeros(2 * 80, np.int32)

    def join(arrs, p=None, to=None, cap=out.size, lens=None):
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[v.ctypes.data for v in arrs])
        ns = np.asarray([len(v) for v in arrs] if lens is None else lens, np.int32)
        return lib.bark_hip_join_many(h, ptrs, ns.ctypes.data, len(arrs), None if p is None else C.byref(p), None if to is None else C.byref(to), out.ctypes.data, cap, lay.ctypes.data)

    good = ctx.join_many([x, x], rate=8000, fmt="mulaw")
    assert join([]) == -1 and join([x] * 65) == -1 and join([x] * 64, cap=0) == -2 - 4 * (64 * 3000 + 63 * 6000)
    assert join([x, x], lens=[3000, 0]) == -1 and join([x], lens=[ofr.MAX_SAMPLES + 1]) == -1
    for bad in (np.nan, np.inf):
        y = x.copy(); y[1234] = bad
        assert join([x, y]) == -1
    assert join([x], to=pkg.audio_format(11025, 0)) == -1 and join([x], to=pkg.audio_format(8000, 3)) == -1 and join([x], to=pkg.audio_format(8000, -1)) == -1
    for p in (_jp(gap_samples=-1), _jp(fade_samples=-1), _jp(trim_pad_frames=-1), _jp(fade_samples=24001), _jp(trim_threshold=float("nan")), _jp(trim_threshold=-0.5),
              _jp(trim_threshold=float("inf"))):
        assert join([x, x], p) == -1
    assert join([x], _jp(fade_samples=24000)) == 12000
    big = np.zeros(ofr.MAX_SAMPLES, np.float32)                                                # 26 x 1 310 720 > 2^25: refused before any work
    assert join([big] * 26, _jp(gap_samples=0)) == -1 and join([x, x], _jp(gap_samples=(1 << 25) - 5999)) == -1
    mu = pkg.audio_format(8000, 2)
    n_mu = -(-(6000 + 6000) // 3)
    assert join([x, x], to=mu, cap=n_mu - 1) == -2 - n_mu and join([x, x], to=mu, cap=n_mu) == n_mu and out[:n_mu].tobytes() == good.tobytes()
    assert lib.bark_hip_join_many(None, None, None, 1, None, None, out.ctypes.data, 16, None) == -1
    with pytest.raises(ValueError):
        ctx.join_many([x], rate=11025)
    _same("after the refusals", ctx.join_many([x, x], rate=8000, fmt="mulaw"), good)
    assert ctx.time_join(8, 3000, 8000, "mulaw", 2) > 0.0 and ctx.time_join(2, 3000, 24000, "f32", 2) > 0.0
    assert ctx.time_join_activity(8, 3000, 2) > 0.0 and lib.bark_hip_time_join_activity(h, 0, 3000, 1) < 0
    assert lib.bark_hip_time_join(h, 65, 3000, 8000, 0, 1) < 0 and lib.bark_hip_time_join(h, 2, 3000, 11025, 0, 1) < 0
    assert ctx.generate_audio("hello world") and len(ctx.audio_data()) > 0                   # the context still generates


def test_the_longest_joined_signal_needs_64_bit_products(ctx, tables):
    """N = 2^25 at 44100 Hz: m M passes 2^32 (m reaches 61.7 million, M = 80).  The first and the last outputs against the rule on J itself."""
    x = rr.dense_signal(3000, seed=3)
    N = 1 << 25
    got = ctx.join_many([x, x], _jp(gap_samples=N - 6000), 44100, "mulaw")
    n_out = ofr.n_out(N, 24000, 44100)
    assert len(got) == n_out and (n_out - 1) * 80 > 1 << 32
    J = np.zeros(N, np.float32)
    J[:3000] = x
    J[-3000:] = x
    for m in (np.arange(0, 7000), np.arange(n_out - 7000, n_out)):
        _same(f"outputs {m[0]} .. {m[-1]}", got[m], ofr.to_format(ofr.resample(J, 24000, 44100, m=m, h=tables[44100]), ofr.MULAW))
    assert np.all(got[20000:40000] == 0xFF)                                                     # the gap: mu-law of +0


# ---- L1: generate_long ---------------------------------------------------------------------------------------------------------------------------------------
def _count(ctx):
    return lambda span: len(ctx.bert_tokenize(span.decode("utf-8"), 257))


def _chunk_equal(what, got, want):
    assert want is not None, what
    assert got["pcm"].tobytes() == want["pcm"].tobytes() and len(got["pcm"]) > 0, what
    for k in ("semantic", "coarse", "fine"):
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.lock_step_job
@pytest.mark.parametrize("temp", [0.0, 0.7], ids=["greedy", "sampled"])
def test_generate_long_is_one_job_of_the_chunks_and_the_join_of_their_audio(tables, temp):
    raw = LONG_TEXT.encode("utf-8")
    one, other = _load(temp=temp, fine_temp=0.5 if temp else 0.0), _load(temp=temp, fine_temp=0.5 if temp else 0.0)
    try:
        spans = one.split_text(LONG_TEXT, 6)
        assert spans == lfr.split(raw, 6, _count(one)) and len(spans) > 4                     # four sentences; the second is over the budget and splits
        assert one.split_text(LONG_TEXT, 0) == lfr.split(raw, 0, _count(one)) and len(one.split_text(LONG_TEXT, 0)) == 4
        join = dict(gap_samples=600, fade_samples=48, trim_threshold=0.0, trim_pad_frames=0)
        rp = one.request_params(seed=77)
        chunks = one.generate_long(LONG_TEXT, max_tokens=6, join=_jp(**join), params=rp)
        assert len(chunks) == len(spans)
        steps = one.batch_lock_steps()
        assert steps is not None and steps[0] > 0 and steps[0] <= 32 + len(spans)              # ONE job: the chunks travelled together, not 32 steps each
        texts = [raw[b:e].decode("utf-8") for b, e in spans]
        alone = other.generate_batch(texts, params=[other.request_params(seed=(77 + i) & 0xFFFFFFFF) for i in range(len(texts))])
        for i, (g, w) in enumerate(zip(chunks, alone)):
            _chunk_equal(f"chunk {i}", g, w)
            _chunk_equal(f"chunk {i} alone", g, other.generate_batch([texts[i]], params=[other.request_params(seed=77 + i)])[0])
        pcm = [c["pcm"] for c in chunks]
        _same("24000 f32", one.long_audio_as(), lfr.joined(pcm, join))
        _same("8000 mu-law", one.long_audio_as(8000, "mulaw"), lfr.joined(pcm, join, 8000, ofr.MULAW, h=tables[8000]))
        lay = lfr.layout(pcm, join)[0]
        assert one.long_chunks() == [(b, e, f, k) for (b, e), (f, k) in zip(spans, lay)]
        # seeds wrap in uint32; a text without a word runs as one chunk; a refused text holds no result
        wrap = one.generate_long("go there. yes", params=one.request_params(seed=0xFFFFFFFF))
        _chunk_equal("wrapped seed", wrap[1], other.generate_batch(["yes"], params=[other.request_params(seed=0)])[0])
        # long_chunks in front of any long_audio_as: the layout alone, without and with a trim threshold
        for jp in (dict(lfr.DEFAULT_JOIN), dict(gap_samples=10, fade_samples=0, trim_threshold=0.01, trim_pad_frames=1)):
            two = one.generate_long("go there. yes", join=_jp(**jp), params=one.request_params(seed=9))
            lay = lfr.layout([c["pcm"] for c in two], jp)[0]
            assert one.long_chunks() == [(0, 9, *lay[0]), (10, 13, *lay[1])], jp
            _same("the join behind the layout", one.long_audio_as(), lfr.joined([c["pcm"] for c in two], jp))
        assert len(one.generate_long("  \n ")) == 1
        with pytest.raises(RuntimeError):
            one.generate_long("a. " * 65)
        with pytest.raises(RuntimeError):
            one.long_audio_as()
        assert one._lib.bark_hip_generate_long(one._h, b"x", C.byref(_pkg().BarkHipLongParams(0, 2, _jp())), None, None, None) == -1
    finally:
        one.free(); other.free()


@pytest.mark.concurrency
def test_request_batcher_joins_long_texts_among_ordinary_requests(tables):
    """two job streams; three long requests mixed with four ordinary ones: each long answer is generate_long + long_audio_as on a fresh context, the
    ordinary answers are what they are without the long ones in the queue"""
    pkg = _pkg()
    join = dict(gap_samples=300, fade_samples=24, trim_threshold=0.0, trim_pad_frames=0)
    longs = [(LONG_TEXT, 6, 11, pkg.audio_format(8000, "mulaw")), ("hello world. this is bark! go there? yes", 0, 21, None),
             (LONG_TEXT, 0, 31, pkg.audio_format(44100, "s16"))]
    plain = ["hello world this is bark", "another one", "third", "and a fourth"]
    owner, fresh = _load(temp=0.7, fine_temp=0.5), _load(temp=0.7, fine_temp=0.5)
    try:
        with pkg.Batcher(owner, max_batch=8, max_wait_ms=50, streams=2) as b:
            tickets, pt = [], []
            for k in range(4):
                if k < 3:
                    text, mt, seed, fmt = longs[k]
                    tickets.append(b.submit(text, seed=seed, audio_format=fmt, long=pkg.BarkHipLongParams(mt, 0, _jp(**join))))
                pt.append(b.submit(plain[k], seed=90 + k))
            assert b._lib.bark_hip_batcher_submit_long(b._b, b"a b", C.byref(pkg.BarkHipLongParams(0, 1, _jp())), None, None, None, None) == -1      # chain
            assert b._lib.bark_hip_batcher_submit_long(b._b, b"a b", C.byref(pkg.BarkHipLongParams(256, 0, _jp())), None, None, None, None) == -1
            # a long text whose every chunk is trimmed away is a legal answer of 0 bytes, in any format and through either wait
            mute = pkg.BarkHipLongParams(0, 0, _jp(trim_threshold=1e30))
            silent = [b.submit("hello world. yes", seed=3, audio_format=pkg.audio_format(8000, "mulaw"), long=mute), b.submit("hello world. yes", seed=3, long=mute)]
            assert [b._lib.bark_hip_batcher_ticket_chunks(b._b, t) for t in tickets + pt[:1] + silent] == [5, 4, 4, 1, 2, 2]
            got = [b.wait_bytes(t) for t in tickets]
            ordinary = [b.wait(t) for t in pt]
            empty = [b.wait_bytes(silent[0]), b.wait(silent[1])]
            assert [len(e) for e in empty] == [0, 0] and empty[0].dtype == np.uint8 and empty[1].dtype == np.float32
            assert b._lib.bark_hip_batcher_ticket_chunks(b._b, tickets[0]) == -1                # a ticket that was waited for is gone
        for k, (text, mt, seed, fmt) in enumerate(longs):
            fresh.generate_long(text, max_tokens=mt, join=_jp(**join), params=fresh.request_params(seed=seed))
            want = fresh.long_audio_as() if fmt is None else fresh.long_audio_as(fmt.sample_rate, {1: "s16", 2: "mulaw"}[fmt.sample_format])
            _same(f"long request {k}", got[k], want)
        alone = fresh.generate_batch(plain, params=[fresh.request_params(seed=90 + k) for k in range(4)])
        for k in range(4):
            assert ordinary[k].tobytes() == alone[k]["pcm"].tobytes() and len(ordinary[k]) > 0, k
    finally:
        owner.free(); fresh.free()


def _post(port, body):
    """(status, headers, body) of POST /bark"""
    import json
    import urllib.error
    import urllib.request
    req = urllib.request.Request(f"http://127.0.0.1:{port}/bark", data=json.dumps(body).encode(), method="POST")
    try:
        with urllib.request.urlopen(req, timeout=200) as r:
            return r.status, dict(r.headers.items()), r.read()
    except urllib.error.HTTPError as e:
        return e.code, dict(e.headers.items()), e.read()


@pytest.mark.concurrency
def test_native_batch_server_long_texts():
    """POST /bark with "long": true at 16000 s16: the WAV's samples are the native call's, X-Bark-Chunks says how many chunks; the same text without "long"
    gives what it gave before; the defaults come from --long / --max-tokens / --gap-ms"""
    import struct
    from tools.make_synth_model import ensure_model
    from test_gpu_output_format import _chunks
    from test_gpu_voice_from_audio import _Server
    model = ensure_model("toy", 0)
    fields = {"text": LONG_TEXT, "seed": 7, "sample_rate": 16000, "format": "s16"}
    with _Server("-m", model) as srv:
        st, head, wav = _post(srv.port, dict(fields, long=True, max_tokens=6, gap_ms=100))
        assert st == 200 and head.get("X-Bark-Chunks") == "5", (st, head)
        st, head1, wav1 = _post(srv.port, dict(fields, long=True))
        assert st == 200 and head1.get("X-Bark-Chunks") == "4"
        st, head0, short = _post(srv.port, {"text": LONG_TEXT, "seed": 7})
        assert st == 200 and "X-Bark-Chunks" not in head0
        st, _, off = _post(srv.port, {"text": LONG_TEXT, "seed": 7, "long": False})
        assert st == 200 and off == short
        for bad in (dict(long=1), dict(long="yes"), dict(long=True, max_tokens=256), dict(long=True, max_tokens=-1), dict(long=True, gap_ms=-1),
                    dict(long=True, gap_ms=1.5), dict(long=True, gap_ms=60001)):
            assert _post(srv.port, dict(fields, **bad))[0] == 400, bad
        assert _post(srv.port, {"text": "a. " * 65, "long": True})[0] == 400                  # more than 64 chunks
    with _Server("-m", model, "--long", "--max-tokens", "6", "--gap-ms", "100", "--sample-rate", "16000", "--format", "s16") as srv:
        st, head2, wav2 = _post(srv.port, {"text": LONG_TEXT, "seed": 7})
        assert st == 200 and head2.get("X-Bark-Chunks") == "5" and wav2 == wav
    one = _load(n_steps_text_encoder=768)
    try:
        one.generate_long(LONG_TEXT, max_tokens=6, join=_jp(gap_samples=2400), params=one.request_params(seed=7))
        want = one.long_audio_as(16000, "s16")
        one.generate_long(LONG_TEXT, params=one.request_params(seed=7))                       # the defaults: one sentence per chunk, 250 ms
        want1 = one.long_audio_as(16000, "s16")
        alone = one.generate_batch([LONG_TEXT], params=[one.request_params(seed=7)])[0]["pcm"]
    finally:
        one.free()
    ch = _chunks(wav)
    assert struct.unpack("<HHIIHH", ch[b"fmt "]) == (1, 1, 16000, 32000, 2, 16) and ch[b"data"] == want.tobytes() and len(want) > 0
    assert _chunks(wav1)[b"data"] == want1.tobytes() and want1.tobytes() != want.tobytes()
    ch = _chunks(short)
    assert struct.unpack("<HHIIHH", ch[b"fmt "]) == (3, 1, 24000, 96000, 4, 32) and ch[b"data"] == alone.tobytes() and len(alone) > 0


@pytest.mark.lock_step_job
def test_chained_chunks_continue_the_voice_of_the_chunk_before():
    pkg = _pkg()
    text = "hello world. this is bark. the river is water"
    one, other = _load(temp=0.7, fine_temp=0.5, n_steps_text_encoder=48), _load(temp=0.7, fine_temp=0.5, n_steps_text_encoder=48)
    try:
        chunks = one.generate_long(text, chain=True, params=one.request_params(seed=5))
        texts = ["hello world.", "this is bark.", "the river is water"]
        assert len(chunks) == 3
        voice, derived = None, []
        for i, t in enumerate(texts):
            want = other.generate_batch([t], params=[other.request_params(seed=5 + i)], voices=[voice])[0]
            _chunk_equal(f"chained chunk {i}", chunks[i], want)
            v = pkg.VoicePrompt(want["semantic"], want["coarse"], want["fine"])
            try:                                                                              # what bark_hip_set_voice_prompt refuses, the chain skips
                other.set_voice_prompt(v); other.set_voice_prompt(None)
                voice = v
                derived.append(i)
            except Exception:
                pass
        assert derived and min(derived) < 2                                                   # the chain did hand a voice on to a later chunk
        k = min(derived) + 1                                                                  # the first chunk that spoke with a derived voice
        flat = one.generate_long(text, chain=False, params=one.request_params(seed=5))
        for i in range(k):
            _chunk_equal(f"chunk {i} is the same in both modes", flat[i], chunks[i])
        assert not np.array_equal(flat[k]["semantic"], chunks[k]["semantic"]) or flat[k]["pcm"].tobytes() != chunks[k]["pcm"].tobytes()
    finally:
        one.free(); other.free()
