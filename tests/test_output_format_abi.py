"""The interface of the output rate and sample format (rule C14r) exists at every layer: exported by libbark.so, declared in include/bark_mi355x.h, mirrored in
bark.cpp_amd/api.py and voice.py, served by bark_batch_server; and what needs no device: the lengths, the tables against the formula, the refusals, and the
three WAV headers of bark.cpp_amd/examples/http_util.h through tests/output_format_driver.cpp."""
import ast
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import output_format_ref as ofr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_resample_out_len", "bark_hip_resample_table", "bark_hip_resample", "bark_hip_resample_many", "bark_hip_get_audio_as", "bark_hip_batch_audio_as",
           "bark_hip_batcher_submit_as", "bark_hip_batcher_wait_bytes", "bark_hip_time_resample_pair"]
METHODS = ["resample", "resample_many", "audio_as", "batch_audio_as", "time_resample_pair"]


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def test_symbols_are_exported_by_the_library():
    lib = os.path.join(ROOT, "bark.cpp_amd", "lib", "libbark.so")
    if not os.path.exists(lib):
        pytest.fail(f"{lib} is missing: build() makes it")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert [s for s in SYMBOLS if s not in exported] == []


def test_symbols_and_structs_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    for s in SYMBOLS:
        assert re.search(rf"BARK_API (int|int64_t|double) {s}\(", text), s
    assert re.search(r"enum bark_hip_sample_format \{ BARK_HIP_SAMPLE_F32 = 0, BARK_HIP_SAMPLE_S16 = 1, BARK_HIP_SAMPLE_MULAW = 2 \};", text)
    assert re.search(r"struct bark_hip_audio_format \{ int32_t sample_rate; int32_t sample_format; \};", text)
    assert "bark_hip_audio_format" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_symbols_are_mirrored_in_python():
    pkg = _pkg()
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    classes = {n.name: {f.name for f in n.body if isinstance(f, ast.FunctionDef)} for n in ast.parse(src).body if isinstance(n, ast.ClassDef)}
    assert [m for m in METHODS if m not in classes["BarkContext"]] == [] and "wait_bytes" in classes["Batcher"]
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in pkg.api.EXPORTS and getattr(lib, s).argtypes is not None, s
    assert lib.bark_hip_time_resample_pair.restype is C.c_double and lib.bark_hip_batcher_submit_as.restype is C.c_int64
    assert C.sizeof(pkg.api.BarkHipAudioFormat) == 8 and [n for n, _ in pkg.api.BarkHipAudioFormat._fields_] == ["sample_rate", "sample_format"]
    f = pkg.audio_format(8000, "mulaw")
    assert (f.sample_rate, f.sample_format) == (8000, 2) and pkg.api.SAMPLE_FORMATS == {"f32": 0, "s16": 1, "mulaw": 2}
    assert "rate" in pkg.voice.from_audio_native.__code__.co_varnames


def test_out_len_for_every_pair():
    lib = _pkg().load_library()
    for a, b in ofr.PAIRS + [(24000, 24000)]:
        for n in (1, 2, 3, 1000, 1310720):
            assert lib.bark_hip_resample_out_len(n, a, b) == ofr.n_out(n, a, b) == -((-n * b) // a), (n, a, b)
        assert lib.bark_hip_resample_out_len(0, a, b) == 0 and lib.bark_hip_resample_out_len(-1, a, b) == -1
    for a, b in ((11025, 24000), (24000, 11025), (16000, 48000), (16000, 16000), (0, 24000), (24000, -8000)):
        assert lib.bark_hip_resample_out_len(100, a, b) == -1, (a, b)


def test_tables_equal_the_formula_and_the_committed_c13r_table():
    """Both sides evaluate the same double-precision expression and are a few double ulps from the true value, so after the rounding to f32 they differ
    by at most one f32 ulp per tap (where libm and numpy agree - as they do on glibc - they are equal)."""
    lib = _pkg().load_library()
    total = 0
    for a, b in ofr.PAIRS:
        lmh = np.zeros(3, np.int32)
        n = lib.bark_hip_resample_table(a, b, None, 0, lmh.ctypes.data)
        assert tuple(int(v) for v in lmh) == ofr.lmh(a, b) and n == int(lmh[0]) * 2 * int(lmh[2])
        got = np.zeros(n, np.float32)
        assert lib.bark_hip_resample_table(a, b, got.ctypes.data, n - 1, lmh.ctypes.data) == -1              # capacity
        assert lib.bark_hip_resample_table(a, b, got.ctypes.data, n, None) == n
        want = ofr.taps(a, b).reshape(-1)
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp), (a, b)
        assert np.array_equal(got == 0.0, want == 0.0)
        total += n
    assert total == 9768
    c13 = np.zeros(44, np.float32)
    assert lib.bark_hip_resample_taps(c13.ctypes.data) == 44
    got = np.zeros(44, np.float32)
    assert lib.bark_hip_resample_table(24000, 16000, got.ctypes.data, 44, None) == 44 and got.tobytes() == c13.tobytes()
    for a, b in ((24000, 24000), (11025, 24000), (16000, 48000)):
        assert lib.bark_hip_resample_table(a, b, got.ctypes.data, 44, None) == -1


def test_entry_points_fail_cleanly_without_a_context_or_arrays():
    pkg = _pkg()
    lib = pkg.load_library()
    x = np.zeros(1000, np.float32)
    out = np.zeros(4000, np.float32)
    to = pkg.audio_format(16000, "s16")
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    n = np.array([1000], np.int32)
    assert lib.bark_hip_resample(None, x.ctypes.data, 1000, 24000, 16000, out.ctypes.data, 4000) == -1
    assert lib.bark_hip_resample_many(None, ptrs, n.ctypes.data, 1, 24000, C.byref(to), out.ctypes.data, 16000, None) == -1
    assert lib.bark_hip_get_audio_as(None, C.byref(to), out.ctypes.data, 16000) == -1
    assert lib.bark_hip_batch_audio_as(None, 0, C.byref(to), out.ctypes.data, 16000) == -1
    assert lib.bark_hip_batcher_submit_as(None, b"x", None, None, None, C.byref(to)) == -1
    assert lib.bark_hip_batcher_wait_bytes(None, 1, out.ctypes.data, 16000) == -1
    assert lib.bark_hip_time_resample_pair(None, 1000, 24000, 16000, 0, 1) < 0


def test_the_server_has_the_fields_and_options():
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    for word in ('"--sample-rate"', '"--format"', '"--voice-audio-resample"', '"sample_rate"', '"resample"', "bark_hip_batcher_submit_as", "bark_hip_batcher_wait_bytes",
                 "bark_hip_resample(encoder_ctx", "wav_samples"):
        assert word in src, word
    # an unsupported format is refused before a default seed is drawn
    assert src.index("format_valid(af)") < src.index("next_seed.fetch_add(1)")


# ---- the three WAV headers -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("output_format") / "driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "bark.cpp_amd", "examples"), os.path.join(ROOT, "tests", "output_format_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _chunks(wav):
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE" and struct.unpack_from("<I", wav, 4)[0] == len(wav) - 8
    out, pos = [], 12
    while pos + 8 <= len(wav):
        size = struct.unpack_from("<I", wav, pos + 4)[0]
        out.append((wav[pos:pos + 4], wav[pos + 8:pos + 8 + size]))
        pos += 8 + size + (size & 1)
    assert pos == len(wav)
    return out


@pytest.mark.parametrize("name,rate,n", [("f32", 24000, 5), ("f32", 44100, 1), ("s16", 16000, 7), ("s16", 48000, 1), ("mulaw", 8000, 6), ("mulaw", 8000, 7), ("mulaw", 8000, 1)])
def test_wav_headers(driver, tmp_path, name, rate, n):
    dt = ofr.DTYPE[{"f32": ofr.F32, "s16": ofr.S16, "mulaw": ofr.MULAW}[name]]
    data = (np.arange(n) * 37 + 5).astype(dt).tobytes()
    src, dst = tmp_path / "in.raw", tmp_path / "out.wav"
    src.write_bytes(data)
    r = subprocess.run([driver, "wav", name, str(rate), str(src), str(dst)], capture_output=True, text=True, timeout=60)
    wav = dst.read_bytes()
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(n), str(len(wav))], r.stdout + r.stderr
    ch = _chunks(wav)
    width = np.dtype(dt).itemsize
    if name == "mulaw":
        assert [c[0] for c in ch] == [b"fmt ", b"fact", b"data"]
        assert struct.unpack("<HHIIHHH", ch[0][1]) == (7, 1, rate, rate, 1, 8, 0) and struct.unpack("<I", ch[1][1]) == (n,)
        assert len(wav) % 2 == 0                                   # an odd data chunk is padded
    else:
        assert [c[0] for c in ch] == [b"fmt ", b"data"]
        assert struct.unpack("<HHIIHH", ch[0][1]) == (3 if name == "f32" else 1, 1, rate, rate * width, width, 8 * width)
    assert ch[-1][1] == data


def test_unknown_format_name(driver, tmp_path):
    (tmp_path / "in.raw").write_bytes(b"\0\0")
    r = subprocess.run([driver, "wav", "alaw", "8000", str(tmp_path / "in.raw"), str(tmp_path / "o.wav")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("err")
