"""The interface of long-form text (rules C15s and C15j) exists at every layer: exported by libbark.so, declared in include/bark_mi355x.h, mirrored in
bark.cpp_amd/api.py with the declared argument types; and what needs no device: the struct sizes, the entry points without a context."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_split_text", "bark_hip_generate_long", "bark_hip_long_audio_as", "bark_hip_long_chunks", "bark_hip_long_chunk_audio", "bark_hip_long_chunk_tokens",
           "bark_hip_join_many", "bark_hip_time_join", "bark_hip_batcher_submit_long", "bark_hip_batcher_ticket_chunks", "bark_hip_time_join_activity"]
METHODS = ["split_text", "generate_long", "long_audio_as", "long_chunks", "join_many", "time_join"]


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


def _c_args(text, name):
    """the parameter list of a declaration, comments and line breaks removed"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(rf"BARK_API (int|int64_t|double) {name}\((.*?)\);", text, flags=re.S)
    assert m, name
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype_of(arg):
    if "*" in arg:
        if arg.startswith("const char *"):
            return "char_p"
        return "pointer"
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}[arg.split()[0]]


def test_symbols_and_structs_are_declared_in_the_header_with_the_mirrored_argument_types():
    pkg = _pkg()
    text = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    lib = pkg.load_library()
    for s in SYMBOLS:
        ret, args = _c_args(text, s)
        fn = getattr(lib, s)
        assert s in pkg.api.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == len(args), (s, args)
        assert (fn.restype is C.c_double) == (ret == "double") and (fn.restype is C.c_int64) == (ret == "int64_t"), s
        for a, t in zip(args, fn.argtypes):
            want = _ctype_of(a)
            if want == "char_p":
                assert t is C.c_char_p, (s, a)
            elif want == "pointer":
                assert t is C.c_void_p or issubclass(t, C._Pointer), (s, a)
            else:
                assert t is want or (C.sizeof(t) == C.sizeof(want) and t in (C.c_int, C.c_int32)), (s, a)
    body = re.search(r"struct bark_hip_join_params \{(.*?)\};", text, flags=re.S).group(1)
    assert re.findall(r"(int32_t|float)\s+(\w+);", body) == [("int32_t", "gap_samples"), ("int32_t", "fade_samples"), ("float", "trim_threshold"), ("int32_t", "trim_pad_frames")]
    assert re.search(r"struct bark_hip_long_params \{ int32_t max_tokens; int32_t chain; struct bark_hip_join_params join; \};", text)
    assert "bark_hip_join_params" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_structs_and_methods_are_mirrored_in_python():
    pkg = _pkg()
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    classes = {n.name: {f.name for f in n.body if isinstance(f, ast.FunctionDef)} for n in ast.parse(src).body if isinstance(n, ast.ClassDef)}
    assert [m for m in METHODS if m not in classes["BarkContext"]] == [] and "long" in pkg.Batcher.submit.__code__.co_varnames
    J, L = pkg.api.BarkHipJoinParams, pkg.api.BarkHipLongParams
    assert C.sizeof(J) == 16 and [n for n, _ in J._fields_] == ["gap_samples", "fade_samples", "trim_threshold", "trim_pad_frames"]
    assert C.sizeof(L) == 24 and [n for n, _ in L._fields_] == ["max_tokens", "chain", "join"] and L.join.offset == 8
    d = pkg.join_params()
    assert (d.gap_samples, d.fade_samples, d.trim_threshold, d.trim_pad_frames) == (6000, 0, 0.0, 0)


def test_entry_points_fail_cleanly_without_a_context():
    pkg = _pkg()
    lib = pkg.load_library()
    x = np.zeros(1000, np.float32)
    out = np.zeros(4000, np.float32)
    ints = np.zeros(256, np.int32)
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    n = np.array([1000], np.int32)
    p = C.POINTER(C.c_float)()
    assert lib.bark_hip_split_text(None, b"a b. c", 0, ints.ctypes.data, 64) == -1
    assert lib.bark_hip_generate_long(None, b"a b. c", None, None, None, None) == -1
    assert lib.bark_hip_long_audio_as(None, None, out.ctypes.data, 16000) == -1
    assert lib.bark_hip_long_chunks(None, ints.ctypes.data, 64) == -1
    assert lib.bark_hip_long_chunk_audio(None, 0, C.byref(p)) == -1
    assert lib.bark_hip_long_chunk_tokens(None, 0, 0, ints.ctypes.data, 256) == -1
    assert lib.bark_hip_join_many(None, ptrs, n.ctypes.data, 1, None, None, out.ctypes.data, 16000, None) == -1
    assert lib.bark_hip_time_join(None, 8, 1000, 8000, 0, 1) < 0
    assert lib.bark_hip_batcher_submit_long(None, b"a b. c", None, None, None, None, None) == -1
