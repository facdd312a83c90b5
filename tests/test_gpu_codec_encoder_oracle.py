"""The EnCodec encoder of the engine against the CPU oracle's (oracle/bark_oracle.cpp: codec_encode_latent, rvq_encode), bit for bit: every tap and the
codes, in both convolution orders (C9m, and C9 under BARK_HIP_CROSSCHECK=1024 / set_codec_mfma(False)), one recording and a full batch of 32, at toy and
EnCodec-24 kHz widths (E1 - E4); and the RVQ kernel against both statements of C11q (numpy: codec_encoder_ref.rvq_c11q, scalar C++: Oracle.rvq_encode) on
the inputs where the rule can go wrong: exact ties, midpoints of two rows, scaled midpoints (A1 - A3).  The oracle's encoder is pinned to numpy and
HuggingFace without a GPU by tests/test_oracle_codec_encoder.py, which also holds the conditions that keep A2 from being blind."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import codec_encoder_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.boundary]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E1_LENGTHS = (1, 7, 319, 320, 321, 977, 2561, 24000)
RAGGED = (1, 320, 977, 2000, 321)


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _model(preset):
    from tools.make_synth_model import ensure_model
    return ensure_model(preset, 0)


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
    """contexts and oracles per model file, made on first use and shared by the tests of the module"""

    def __init__(self, tmp):
        self.tmp, self.ctxs, self.orcs, self.tie = tmp, {}, {}, None

    def ctx(self, path):
        if path not in self.ctxs:
            pkg = _pkg()
            self.ctxs[path] = pkg.BarkContext.load_model(path, pkg.default_params(temp=0.0, fine_temp=0.0, n_steps_text_encoder=32), seed=0)
        return self.ctxs[path]

    def oracle(self, path):
        if path not in self.orcs:
            from oracle.pyoracle import Oracle
            self.orcs[path] = Oracle(path, n_threads=8)
        return self.orcs[path]

    def tie_model(self):
        """(path, codebooks) of the toy_enc file with duplicated codebook rows (ref.write_tie_model)"""
        if self.tie is None:
            dst = os.path.join(self.tmp, "bark_toy_enc_ties.bin")
            self.tie = (dst, ref.write_tie_model(_model("toy_enc"), dst))
        return self.tie

    def close(self):
        for c in self.ctxs.values():
            c.free()
        for o in self.orcs.values():
            o.close()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    e = _Env(str(tmp_path_factory.mktemp("codec_encoder_oracle")))
    yield e
    e.close()


# ---- E1 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E1_LENGTHS, ids=lambda v: f"n{v}_")
def test_taps_and_codes_equal_the_oracle(env, n):
    """toy_enc, default order (C9m where the input channels are a multiple of 8, C9 otherwise): taps 0 - 6 and the codes.  1 and 7 samples take the padding
    rule's short-input detour at every stage, 320 at the last stride only (8 rows, pad 8), 321 not; 2561 gives 2561 / 1281 / 321 / 65 / 9 rows, so the
    last 128-row workgroup of three strided convolutions holds exactly one live lane; 24000 (taps 5, 6 and codes only): 75 frames, the LSTM's captured
    64-step block replays twice."""
    path = _model("toy_enc")
    ctx, orc = env.ctx(path), env.oracle(path)
    orc.set_codec_mfma(True)
    x = ref.fixture_signal(n)
    for st in ((5, 6) if n == 24000 else range(7)):
        _exact(f"toy_enc n={n} encoder tap {st}", ctx.codec_encode_tap(x, st), orc.codec_encode_tap(x, st))
    _exact(f"toy_enc n={n} codes", ctx.codec_encode(x, 8), orc.codec_encode(x, 8))


# ---- E2 / E4 ----------------------------------------------------------------------------------------------------------------------------------------
_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import codec_encoder_ref as ref
from bark_amd_loader import load_package
pkg = load_package()
ctx = pkg.BarkContext.load_model(sys.argv[2], pkg.default_params(temp=0.0, fine_temp=0.0), 0)
d = {}
for n in (int(v) for v in sys.argv[3].split(",")):
    x = ref.fixture_signal(n)
    for st in (int(v) for v in sys.argv[4].split(",")):
        d["tap%%d_n%%d" %% (st, n)] = ctx.codec_encode_tap(x, st)
    d["codes_n%%d" %% n] = ctx.codec_encode(x, 8)
np.savez(sys.argv[1], **d)
ctx.free()
''' % (ROOT, os.path.join(ROOT, "tests"))


def _both_orders_in_child_processes(env, preset, lengths, stages):
    """one fresh process per order (the mask BARK_HIP_CROSSCHECK is read once per process), one after the other; each against the oracle in that order"""
    path = _model(preset)
    orc = env.oracle(path)
    try:
        for flag, mfma in (("0", True), ("1024", False)):
            with tempfile.NamedTemporaryFile(suffix=".npz", delete=False, dir=env.tmp) as f:
                out = f.name
            r = subprocess.run([sys.executable, "-c", _CHILD, out, path, ",".join(map(str, lengths)), ",".join(map(str, stages))],
                               env=dict(os.environ, BARK_HIP_CROSSCHECK=flag), capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-1500:]
            got = np.load(out)
            orc.set_codec_mfma(mfma)
            for n in lengths:
                x = ref.fixture_signal(n)
                for st in stages:
                    _exact(f"{preset} n={n} encoder tap {st}, codec_mfma={mfma}", got[f"tap{st}_n{n}"], orc.codec_encode_tap(x, st))
                _exact(f"{preset} n={n} codes, codec_mfma={mfma}", got[f"codes_n{n}"], orc.codec_encode(x, 8))
    finally:
        orc.set_codec_mfma(True)


@pytest.mark.parametrize("lengths", [(1, 7, 321), (319, 320, 977, 2561)], ids=lambda v: "n" + "_".join(map(str, v)) + "_")
def test_both_convolution_orders_equal_the_oracle(env, lengths):
    """E1's lengths up to 2561 in C9m and, with every convolution sent to the chain kernels (bit 1024), in C9 - conv_tm_chain_kernel and
    conv_down_chain_kernel, the sibling of the strided convolution that no other test runs."""
    _both_orders_in_child_processes(env, "toy_enc", lengths, range(7))


@pytest.mark.parametrize("n", [977, 5161], ids=lambda v: f"n{v}_")
def test_encodec_24khz_widths_equal_the_oracle_in_both_orders(env, n):
    """`small` carries the encoder at EnCodec-24 kHz widths (16 column tiles at 512 output channels); 5161 samples give 130 rows after the third stride:
    two workgroups at kd = 1280.  Taps 1 - 4, the latent and the codes."""
    _both_orders_in_child_processes(env, "small", (n,), (1, 2, 3, 4, 6))


# ---- E3 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [tuple(1 + 37 * b for b in range(32)), RAGGED], ids=["full32", "ragged5"])
def test_batch_equals_the_oracle_recording_by_recording(env, lengths):
    """One codec_encode_many: every recording's codes and its slice of the latents equal the oracle's single-recording result.  32 recordings of
    1 + 37 b samples: the row tables are full and every recording boundary falls inside a wave at every stage."""
    path = _model("toy_enc")
    ctx, orc = env.ctx(path), env.oracle(path)
    orc.set_codec_mfma(True)
    xs = [ref.fixture_signal(24000)[-n:].copy() for n in lengths]          # different content per recording: state leaking between them would show
    many = ctx.codec_encode_many(xs, 8)
    zs = ctx.codec_encode_latents(sum(-(-n // 320) for n in lengths))
    off = 0
    for b, (x, got) in enumerate(zip(xs, many)):
        T = -(-len(x) // 320)
        _exact(f"recording {b} ({len(x)} samples) of {len(xs)}: codes", got, orc.codec_encode(x, 8))
        _exact(f"recording {b} ({len(x)} samples) of {len(xs)}: latents", zs[off:off + T], orc.codec_encode_tap(x, 6).T)
        off += T
    assert off == len(zs)


# ---- A1 - A3 ----------------------------------------------------------------------------------------------------------------------------------------
def _rvq_three_ways(name, ctx, orc, z, cbs, n_q):
    got = ctx.rvq_encode(z, n_q)
    _exact(f"{name}: kernel against numpy C11q", got, ref.rvq_c11q(z, cbs, n_q))
    _exact(f"{name}: kernel against the oracle's C11q", got, orc.rvq_encode(z, n_q))


@pytest.mark.parametrize("n_q", [1, 8], ids=lambda v: f"q{v}")
def test_rvq_kernel_on_exact_ties(env, n_q):
    """A1: codebooks 0 and 3 of a copy of the toy_enc file hold equal rows - in one work-item of the kernel (j, j + 256), in neighbouring lanes (j, j + 1),
    in different waves (j, j + 64), the last row equal to a low one (1023, 5).  Latents: the duplicated row itself (both distances 0), the row plus noise
    (equal non-zero distances), the same behind three other picks (the tie arises at stage 3), the all-zero latent; in calls of 1, 4 and 5 frames (full and
    partial workgroups of four, every latent in every frame slot).  The lowest row must win, as in both reference loops."""
    path, cbs = env.tie_model()
    ctx, orc = env.ctx(path), env.oracle(path)
    z = ref.tie_latents(cbs)
    for T in (1, 4, 5):
        for s in range(0, len(z), T):
            _rvq_three_ways(f"ties, T={T}, latents from {s}", ctx, orc, z[(s + np.arange(T)) % len(z)], cbs, n_q)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 10, 2.0 ** -10], ids=["x1", "x2p10", "x2m10"])
@pytest.mark.parametrize("n_q", [1, 8], ids=lambda v: f"q{v}")
def test_rvq_kernel_on_midpoints(env, n_q, scale):
    """A2 (scale 1): 515 latents f32((e_a + e_b) / 2) for random pairs of the model's own stage-0 rows - 128 full workgroups and one of three frames; in
    exact arithmetic each is equally far from both rows, so the order of the rounded operations alone decides the pick, and the residual carries the
    decision through all eight stages.  Measured on these latents on the CPU (tests/test_oracle_codec_encoder.py::test_midpoint_latents_tell_the_orders_apart,
    which asserts the floors 5 % / 10 %): the stage-0 pick differs from C11q's in 13.6 % of the frames when acc + t t is fused and in 27.4 % when d runs
    downwards - a kernel in either order fails here.  A3 (scales 2^10, 2^-10): the same construction scaled, the pairs recomputed as neighbours in the
    order of the rows' norms (ref.midpoint_latents): magnitudes at which the squares leave the range the codebooks were drawn for."""
    path = _model("toy_enc")
    cbs = ref.codebooks(ref.codec_tensors(path)[1], 8)
    z = ref.midpoint_latents(cbs, 515, scale)
    _rvq_three_ways(f"midpoints x {scale}", env.ctx(path), env.oracle(path), z, cbs, n_q)
