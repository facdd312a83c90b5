"""The semantic encoder's public interface (rule C12h) exists at every layer: exported by libbark.so, declared in include/bark_mi355x.h, mirrored in
bark.cpp_amd/api.py; voice.from_audio keeps its behaviour when the ids are given and refuses without ids and without an encoder."""
import ast
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_load_semantic_encoder", "bark_hip_has_semantic_encoder", "bark_hip_semantic_encode", "bark_hip_semantic_encode_tap", "bark_hip_semantic_head",
           "bark_hip_semantic_encode_device_us"]
METHODS = ["load_semantic_encoder", "has_semantic_encoder", "semantic_encode", "semantic_encode_tap", "semantic_head"]


def test_symbols_are_exported_by_the_library():
    lib = os.path.join(ROOT, "bark.cpp_amd", "lib", "libbark.so")
    if not os.path.exists(lib):
        pytest.fail(f"{lib} is missing: build() makes it")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert [s for s in SYMBOLS if s not in exported] == []


def test_symbols_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    for s in SYMBOLS:
        assert re.search(r"BARK_API\s+(int|double)\s+" + s + r"\s*\(", text), s
    assert re.search(r"bark_hip_semantic_encode\(struct bark_context \*\s*\w+, const float \*\s*\w+, int \w+, int32_t \*\s*\w+, int \w+\)", text)
    assert re.search(r"bark_hip_semantic_head\(struct bark_context \*\s*\w+, const float \*\s*\w+, int \w+, int32_t \*\s*\w+, float \*\s*\w+\)", text)


def test_symbols_are_mirrored_in_api_py():
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    tree = ast.parse(src)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BarkContext")
    have = {f.name for f in cls.body if isinstance(f, ast.FunctionDef)}
    assert [m for m in METHODS if m not in have] == []
    for s in SYMBOLS:
        assert f"lib.{s}.argtypes" in src and f'"{s}"' in src, s
    assert "lib.bark_hip_semantic_encode_device_us.restype = C.c_double" in src


class _FakeCtx:
    def __init__(self, has):
        self.has, self.encoded = has, []

    def codec_encode(self, pcm, n_q):
        return np.arange(8 * 5, dtype=np.int32).reshape(8, 5)

    def has_semantic_encoder(self):
        return self.has

    def semantic_encode(self, x):
        self.encoded.append(np.asarray(x))
        return np.array([7, 8, 9], np.int32)


def test_from_audio_with_and_without_ids():
    spec = importlib.util.spec_from_file_location("bark_voice_for_abi", os.path.join(ROOT, "bark.cpp_amd", "voice.py"))
    voice = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(voice)
    pcm = np.zeros(1600, np.float32)
    sem = np.array([3, 1, 4], np.int32)
    for ctx in (_FakeCtx(False), _FakeCtx(True)):                  # ids given: exactly as before, the encoder is not consulted
        v = voice.from_audio(ctx, pcm, sem)
        assert np.array_equal(v.semantic, sem) and v.fine.shape == (5, 8) and np.array_equal(v.coarse, v.fine[:, :2]) and ctx.encoded == []
        assert voice.from_audio(ctx, pcm, semantic=sem) == v
    with pytest.raises(ValueError):
        voice.from_audio(_FakeCtx(False), pcm)
    ctx = _FakeCtx(True)
    v = voice.from_audio(ctx, pcm)
    assert np.array_equal(v.semantic, [7, 8, 9]) and len(ctx.encoded) == 1 and len(ctx.encoded[0]) == -(-2 * 1600 // 3)
    assert np.array_equal(ctx.encoded[0], voice.resample_24k_to_16k(pcm))
