"""The interface of voice prompts from a recording (rule C13r) exists at every layer: exported by libbark.so with the declared signatures, declared in
include/bark_mi355x.h, mirrored in bark.cpp_amd/api.py and voice.py, served by bark_batch_server; and the refusals that need no device."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_resample_taps", "bark_hip_resample_24k_to_16k", "bark_hip_voice_from_audio", "bark_hip_set_voice_from_audio", "bark_hip_time_resample"]
METHODS = ["resample_24k_to_16k", "voice_from_audio", "set_voice_from_audio", "time_resample"]


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


def test_symbols_are_declared_in_the_header_with_their_signatures():
    text = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    ctx, fl, i32 = r"struct bark_context \*\s*\w+", r"const float \*\s*\w+", r"int32_t \*\s*\w+"
    for pattern in (r"BARK_API int bark_hip_resample_taps\(float \*\s*\w+\);",
                    rf"BARK_API int bark_hip_resample_24k_to_16k\({ctx}, {fl}, int \w+, float \*\s*\w+, int \w+\);",
                    rf"BARK_API int bark_hip_voice_from_audio\({ctx}, {fl}, int \w+, {i32}, int \w+,\s*{i32}, {i32}, int \w+, {i32}, {i32}\);",
                    rf"BARK_API int bark_hip_set_voice_from_audio\({ctx}, {fl}, int \w+\);",
                    rf"BARK_API double bark_hip_time_resample\({ctx}, int \w+, int \w+\);",
                    r"#define BARK_HIP_VOICE_AUDIO_MAX_SAMPLES 480000\b"):
        assert re.search(pattern, text), pattern
    assert "voice_from_audio" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_symbols_are_mirrored_in_python():
    pkg = _pkg()
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "BarkContext")
    have = {f.name for f in cls.body if isinstance(f, ast.FunctionDef)}
    assert [m for m in METHODS if m not in have] == []
    lib = pkg.load_library()
    vp = C.c_void_p
    want = {"bark_hip_resample_taps": [vp], "bark_hip_resample_24k_to_16k": [vp, vp, C.c_int, vp, C.c_int],
            "bark_hip_voice_from_audio": [vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp], "bark_hip_set_voice_from_audio": [vp, vp, C.c_int],
            "bark_hip_time_resample": [vp, C.c_int, C.c_int]}
    for s in SYMBOLS:
        assert s in pkg.api.EXPORTS and list(getattr(lib, s).argtypes) == want[s], s
    assert lib.bark_hip_time_resample.restype is C.c_double
    assert pkg.api.VOICE_AUDIO_MAX_SAMPLES == 480000 and callable(pkg.voice.from_audio_native)


def test_entry_points_fail_cleanly_without_a_context_or_arrays():
    lib = _pkg().load_library()
    x = np.zeros(1000, np.float32)
    out = np.zeros(1000, np.float32)
    ids = np.zeros(8000, np.int32)
    n = np.zeros(2, np.int32)
    assert lib.bark_hip_resample_taps(None) == -1
    assert lib.bark_hip_resample_24k_to_16k(None, x.ctypes.data, 1000, out.ctypes.data, 1000) == -1
    assert lib.bark_hip_voice_from_audio(None, x.ctypes.data, 1000, ids.ctypes.data, 100, ids.ctypes.data, ids.ctypes.data, 100, n.ctypes.data, n[1:].ctypes.data) == -1
    assert lib.bark_hip_set_voice_from_audio(None, x.ctypes.data, 1000) == -1
    assert lib.bark_hip_time_resample(None, 1000, 1) < 0


class _FakeCtx:
    def voice_from_audio(self, pcm):
        self.seen = np.asarray(pcm)
        return np.array([7, 8], np.int32), np.arange(8, dtype=np.int32).reshape(4, 2), np.arange(32, dtype=np.int32).reshape(4, 8)


def test_from_audio_native_wraps_the_native_call():
    voice = _pkg().voice
    ctx = _FakeCtx()
    pcm = np.ones(1079, np.float32)
    v = voice.from_audio_native(ctx, pcm)
    assert isinstance(v, voice.VoicePrompt) and ctx.seen is pcm
    assert np.array_equal(v.semantic, [7, 8]) and v.coarse.shape == (4, 2) and v.fine.shape == (4, 8)


def test_the_server_has_the_routes_and_options():
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    for word in ('"--semantic-encoder"', '"--voice-audio"', "POST /voices", "GET /voices", "bark_hip_voice_from_audio", "std::shared_mutex", "shared_ptr<const VoiceFile>", "parse_wav"):
        assert word in src, word
    # the encoder is loaded before the first clone is made
    assert src.index("bark_hip_load_semantic_encoder(ctx") < src.index("bark_hip_clone_context(") < src.index("bark_hip_batcher_create_ex(")
