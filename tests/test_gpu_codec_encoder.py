"""GPU tests of the EnCodec encoder (bark_hip_codec_encode*, bark_hip_rvq_encode, voice.from_audio) against tests/codec_encoder_ref.py (pinned to
HuggingFace by tests/test_codec_encoder_ref.py) and the HF fixtures tests/golden/hf_<preset>_encoder_s0.npz.

Measured on the device (max abs deviation of the latent from HF's f32 latent / allowed 4 x latent_f16emu_maxabs + 1e-5): see DESIGN.md section 3,
"Encoder parity"."""
import os
import subprocess
import sys

import numpy as np
import pytest

import codec_encoder_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(p, n) for p in ("toy_enc", "small") for n in ref.FIXTURE_LENGTHS[p]]
CASE_IDS = [f"{p}-n{n}" for p, n in CASES]


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


class _Env:
    """contexts, tensors and fixtures per preset, made on first use and shared by the tests of the module"""

    def __init__(self):
        self.ctxs, self.tens, self.gold = {}, {}, {}

    def ctx(self, preset):
        if preset not in self.ctxs:
            pkg = _pkg()
            self.ctxs[preset] = pkg.BarkContext.load_model(_model(preset), pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32), seed=0)
        return self.ctxs[preset]

    def tensors(self, preset):
        if preset not in self.tens:
            self.tens[preset] = ref.codec_tensors(_model(preset))[1]
        return self.tens[preset]

    def codebooks(self, preset):
        return ref.codebooks(self.tensors(preset), 8)

    def fixture(self, preset):
        if preset not in self.gold:
            self.gold[preset] = np.load(os.path.join(ROOT, "tests", "golden", f"hf_{preset}_encoder_s0.npz"))
        return self.gold[preset]

    def close(self):
        for c in self.ctxs.values():
            c.free()


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 2, 8], ids=lambda v: f"q{v}")
@pytest.mark.parametrize("T", [1, 4, 33, 75], ids=lambda v: f"T{v}-")
def test_rvq_kernel_equals_c11q(env, T, n_q):
    """bark_hip_rvq_encode against C11q in numpy, exactly.  Latents: sums of random codebook rows plus N(0, 0.3) noise, so the picks are spread over the
    codebooks (T = 4: one full workgroup of frames, 33: a partial last one)."""
    cbs = env.codebooks("toy_enc")
    rng = np.random.default_rng(1000 * T + n_q)
    z = sum(cbs[q][rng.integers(0, cbs.shape[1], T)] for q in range(8)) + 0.3 * rng.standard_normal((T, cbs.shape[2]))
    z = z.astype(np.float32)
    got = env.ctx("toy_enc").rvq_encode(z, n_q)
    want = ref.rvq_c11q(z, cbs, n_q)
    assert got.shape == want.shape == (n_q, T)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} codes differ"
    if T >= 33:
        assert len(np.unique(want[0])) > T // 2           # the picks are spread


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n", CASES, ids=CASE_IDS)
def test_latent_taps_and_decided_codes_against_hf(env, preset, n):
    """The stage-6 tap against HF's f32 latent: max abs deviation <= 4 x latent_f16emu_maxabs + 1e-5 (the fixture's own measure of what rounding
    the operator inputs to f16 does to HF; 4 x: the device also keeps the LSTM state in f16 and accumulates in the matrix cores' order).  Intermediate
    taps (toy_enc): the same bound scaled by max|tap| / max|latent| of the HF activations - an equal RELATIVE bound, so that a failure names its layer.
    Codes: a frame is decided when at every stage HF's margin exceeds 4 |z_gpu[t] - z_hf[t]|_2 max_j |e_qj|; decided frames must carry HF's codes;
    on the 24000-sample inputs at least a third of the frames must be decided."""
    g = env.fixture(preset)
    ctx = env.ctx(preset)
    x = ref.fixture_signal(n)
    z_hf = g[f"latent_n{n}"]
    emu = float(g[f"latent_f16emu_maxabs_n{n}"])
    z = ctx.codec_encode_tap(x, 6)
    assert z.shape == z_hf.shape
    lat_scale = float(np.abs(z_hf).max())
    for st in range(6):
        if f"tap{st}_n{n}" not in g:
            continue
        want = g[f"tap{st}_n{n}"]
        got = ctx.codec_encode_tap(x, st)
        assert got.shape == want.shape, (st, got.shape, want.shape)
        dev = float(np.abs(got - want).max())
        tol = 4.0 * emu * float(np.abs(want).max()) / lat_scale + 1e-5
        print(f"{preset} n={n} tap {st}: max abs dev {dev:.3e}, allowed {tol:.3e}")
        assert dev <= tol, f"tap {st}: {dev:.3e} > {tol:.3e}"
    dev = float(np.abs(z - z_hf).max())
    tol = 4.0 * emu + 1e-5
    print(f"{preset} n={n} latent: max abs dev {dev:.3e}, allowed {tol:.3e} (f16emu {emu:.3e})")
    assert dev <= tol, f"latent: {dev:.3e} > {tol:.3e}"
    # code agreement with HF on the frames the deviation cannot flip
    cbs = env.codebooks(preset)
    codes_hf = g[f"codes_n{n}"]
    codes = ctx.codec_encode(x, 8)
    assert codes.shape == codes_hf.shape
    decided = ref.decided_frames(z.T, z_hf.T, cbs, codes_hf)
    agree = float((codes == codes_hf).mean())
    print(f"{preset} n={n}: {int(decided.sum())} of {len(decided)} frames decided, overall code agreement {agree:.4f}")
    assert np.array_equal(codes[:, decided], codes_hf[:, decided])
    if n == 24000:
        assert decided.mean() >= 1.0 / 3.0, decided.mean()


# ---- G3 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n", CASES, ids=CASE_IDS)
def test_codes_are_c11q_of_the_engines_own_latent(env, preset, n):
    ctx = env.ctx(preset)
    x = ref.fixture_signal(n)
    codes = ctx.codec_encode(x, 8)
    z = ctx.codec_encode_tap(x, 6)
    assert codes.shape == (8, -(-n // 320))
    assert np.array_equal(codes, ref.rvq_c11q(z.T, env.codebooks(preset), 8))
    assert np.array_equal(ctx.codec_encode(x, 3), codes[:3])


# ---- G4 / G5 ----------------------------------------------------------------------------------------------------------------------------------------
RAGGED = (1, 320, 977, 2000, 321)


def _batch_equals_singles(ctx):
    xs = [ref.fixture_signal(n) for n in RAGGED]
    many = ctx.codec_encode_many(xs, 8)
    zs = ctx.codec_encode_latents(sum(-(-n // 320) for n in RAGGED))
    off = 0
    for x, cm in zip(xs, many):
        one = ctx.codec_encode(x, 8)
        T = one.shape[1]
        assert np.array_equal(cm, one), len(x)
        assert np.array_equal(ctx.codec_encode_latents(T), zs[off:off + T]), len(x)
        assert np.array_equal(ctx.codec_encode_tap(x, 6).T, zs[off:off + T]), len(x)
        off += T
    return many


def test_ragged_batch_is_bit_identical_to_single_calls(env):
    _batch_equals_singles(env.ctx("toy_enc"))


def test_clone_encodes_the_same_bits(env):
    ctx = env.ctx("toy_enc")
    cl = ctx.clone(seed=1)
    try:
        assert cl.has_codec_encoder()
        a, b = _batch_equals_singles(cl), ctx.codec_encode_many([ref.fixture_signal(n) for n in RAGGED], 8)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    finally:
        cl.free()


def test_encoder_graph_and_eager_agree():
    """BARK_HIP_GRAPH=0 runs the LSTM's launches one by one instead of replaying the captured block: same codes, same latent (75 frames: two replays)."""
    code = (
        "import sys, hashlib, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import codec_encoder_ref as ref\n"
        "from bark_amd_loader import load_package; pkg = load_package()\n"
        "c = pkg.BarkContext.load_model(%r, pkg.default_params(temp=0.0, fine_temp=0.0), 0)\n"
        "h = hashlib.sha256()\n"
        "for n in (977, 24000):\n"
        "    x = ref.fixture_signal(n); h.update(c.codec_encode(x, 8).tobytes()); h.update(c.codec_encode_tap(x, 6).tobytes())\n"
        "print(h.hexdigest())\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), _model("toy_enc"))
    outs = []
    for graph in ("1", "0"):
        env_ = dict(os.environ, BARK_HIP_GRAPH=graph)
        outs.append(subprocess.run([sys.executable, "-c", code], env=env_, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1]


def test_encode_decode_encode_on_one_context(env):
    """the encoder's and the decoder's captured LSTM blocks live in slots of their own: a decode in between changes nothing"""
    ctx = env.ctx("toy_enc")
    x = ref.fixture_signal(24000)
    first = ctx.codec_encode(x, 8)
    pcm = ctx.codec_decode(first)
    assert pcm.shape == (320 * first.shape[1],) and np.isfinite(pcm).all()
    pcm2 = ctx.codec_decode(first)
    assert np.array_equal(ctx.codec_encode(x, 8), first)
    assert np.array_equal(ctx.codec_decode(first), pcm) and np.array_equal(pcm2, pcm)


# ---- G6 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(env, toy_model):
    ctx = env.ctx("toy_enc")
    lib, h = ctx._lib, ctx._h
    x = ref.fixture_signal(977)
    good = ctx.codec_encode(x, 8)
    codes = np.zeros((8, 8192), np.int32)
    out = np.zeros(1 << 16, np.float32)

    def enc(arr, n, n_q, cap):
        return lib.bark_hip_codec_encode(h, arr.ctypes.data, n, n_q, codes.ctypes.data, cap)
    assert ctx.has_codec_encoder()
    assert enc(x, 0, 8, codes.size) == -1 and enc(x, -5, 8, codes.size) == -1                # n_samples < 1
    long = np.zeros(4096 * 320 + 1, np.float32)
    assert enc(long, len(long), 1, codes.size) == -1                                         # more than 4096 frames
    assert enc(x, len(x), 0, codes.size) == -1 and enc(x, len(x), 9, codes.size) == -1       # n_q outside 1 .. 8
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[500] = bad
        assert enc(y, len(y), 8, codes.size) == -1
        assert lib.bark_hip_codec_encode_tap(h, y.ctypes.data, len(y), 6, out.ctypes.data, out.size) == -1
    # a finite sample whose f16 image is infinite (every convolution reads the f16 image of its input): refused at the door, by all three entry points
    y = x.copy(); y[500] = 1e5
    with np.errstate(over="ignore"):
        assert np.isfinite(y).all() and not np.isfinite(y.astype(np.float16)).all()
    assert enc(y, len(y), 8, codes.size) == -1
    assert lib.bark_hip_codec_encode_tap(h, y.ctypes.data, len(y), 6, out.ctypes.data, out.size) == -1
    for stage in (0, 3):
        assert lib.bark_hip_codec_encode_tap(h, y.ctypes.data, len(y), stage, out.ctypes.data, out.size) == -1
    for where in (0, 1):                                                                     # one bad recording of two, either place
        pair = [x, x]; pair[where] = y
        p2 = (__import__("ctypes").c_void_p * 2)(*[a.ctypes.data for a in pair])
        n2 = np.full(2, len(x), np.int32)
        assert lib.bark_hip_codec_encode_many(h, p2, n2.ctypes.data, 2, 8, codes.ctypes.data, codes.size) == -1
    assert enc(x, len(x), 8, 8 * 4 - 1) == -1                                                # capacity too small
    assert lib.bark_hip_codec_encode_tap(h, x.ctypes.data, len(x), 7, out.ctypes.data, out.size) == -1
    assert lib.bark_hip_codec_encode_tap(h, x.ctypes.data, len(x), 6, out.ctypes.data, 10) == -1
    z = np.zeros((4, 128), np.float32)
    assert lib.bark_hip_rvq_encode(h, z.ctypes.data, 4, 9, codes.ctypes.data) == -1 and lib.bark_hip_rvq_encode(h, z.ctypes.data, 0, 8, codes.ctypes.data) == -1
    # a frame with no finite distance to any codebook row is an error, never a code (C11q): NaN / inf entries, and squares that overflow
    for bad in (np.nan, np.inf, -np.inf, 3e19):
        for T, t in ((4, 2), (5, 4), (1, 0)):
            zb = np.random.default_rng(3).standard_normal((T, 128)).astype(np.float32); zb[t, 7] = bad
            for n_q in (1, 8):
                codes[:] = 0
                assert lib.bark_hip_rvq_encode(h, zb.ctypes.data, T, n_q, codes.ctypes.data) == -1, (bad, T, n_q)
    ptrs = (__import__("ctypes").c_void_p * 33)(*[x.ctypes.data] * 33)
    ns = np.full(33, len(x), np.int32)
    big = np.zeros(33 * 8 * 4, np.int32)
    assert lib.bark_hip_codec_encode_many(h, ptrs, ns.ctypes.data, 33, 8, big.ctypes.data, big.size) == -1      # more than 32 recordings
    assert np.array_equal(ctx.codec_encode(x, 8), good)                                      # still usable, same bits
    # a file without the encoder
    pkg = _pkg()
    toy = pkg.BarkContext.load_model(toy_model, pkg.default_params(temp=0.0, fine_temp=0.0), seed=0)
    try:
        assert not toy.has_codec_encoder() and "codec encoder" not in toy.describe() and "codec encoder" in ctx.describe()
        assert toy._lib.bark_hip_codec_encode(toy._h, x.ctypes.data, len(x), 8, codes.ctypes.data, codes.size) == -1
        assert toy._lib.bark_hip_codec_encode_tap(toy._h, x.ctypes.data, len(x), 6, out.ctypes.data, out.size) == -1
        assert toy._lib.bark_hip_rvq_encode(toy._h, z.ctypes.data, 4, 8, codes.ctypes.data) == -1
        assert toy.codec_decode(good).shape == (320 * good.shape[1],)
    finally:
        toy.free()


def test_decode_of_encode_gives_320_samples_per_frame(env):
    ctx = env.ctx("toy_enc")
    for n in (1, 321, 977):
        codes = ctx.codec_encode(ref.fixture_signal(n), 8)
        pcm = ctx.codec_decode(codes)
        assert pcm.shape == (320 * codes.shape[1],) and np.isfinite(pcm).all()


# ---- G7 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_voice_prompt_from_audio(env):
    pkg = _pkg()
    ctx = env.ctx("toy_enc")
    x = ref.fixture_signal(24000)
    sem = np.random.default_rng(11).integers(0, 10000, 60).astype(np.int32)
    v = pkg.voice.from_audio(ctx, x, sem)
    codes = ctx.codec_encode(x, 8)
    assert v.fine.shape == (75, 8) and v.coarse.shape == (75, 2) and np.array_equal(v.semantic, sem)
    assert np.array_equal(v.fine, codes.T) and np.array_equal(v.coarse, v.fine[:, :2])
    ctx.set_voice_prompt(v)
    try:
        assert ctx.generate_audio("hello world this is bark")
        assert len(ctx.audio_data()) == 320 * len(ctx.fine_tokens()) > 0
    finally:
        ctx.set_voice_prompt(None)
