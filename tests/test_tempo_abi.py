"""The interface of the speaking rate (rule C16t) exists at every layer: exported by libbark.so, declared in include/bark_mi355x.h, mirrored in
bark.cpp_amd/api.py with the declared argument types, spoken by bark_batch_server; and what needs no device: the length function, the window table,
the entry points without a context."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tempo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_tempo_out_len", "bark_hip_tempo_window", "bark_hip_tempo", "bark_hip_tempo_many", "bark_hip_tempo_positions", "bark_hip_get_audio_at",
           "bark_hip_batch_audio_at", "bark_hip_long_audio_at", "bark_hip_batcher_submit_at", "bark_hip_batcher_submit_long_at", "bark_hip_time_tempo"]
METHODS = ["tempo", "tempo_many", "tempo_positions", "audio_at", "batch_audio_at", "long_audio_at", "time_tempo"]


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
        return "char_p" if arg.startswith("const char *") else "pointer"
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}[arg.split()[0]]


def test_symbols_are_declared_in_the_header_with_the_mirrored_argument_types():
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
    assert "speed_permille" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_methods_are_mirrored_in_python():
    pkg = _pkg()
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    classes = {n.name: {f.name for f in n.body if isinstance(f, ast.FunctionDef)} for n in ast.parse(src).body if isinstance(n, ast.ClassDef)}
    assert [m for m in METHODS if m not in classes["BarkContext"]] == [] and "speed" in pkg.Batcher.submit.__code__.co_varnames
    assert [pkg.speed_permille(v) for v in (0.5, 0.667, 0.9995, 1.0, 1.25, 2.0)] == [500, 667, 1000, 1000, 1250, 2000]


def test_out_len_gives_the_rule_and_refuses_what_it_should():
    lib = _pkg().load_library()
    for n in (1, 2, 359, 360, 361, 719, 720, 721, 1081, 122880, tr.MAX_SAMPLES):
        for p in (500, 501, 667, 999, 1000, 1001, 1250, 1999, 2000):
            assert lib.bark_hip_tempo_out_len(n, p) == tr.out_len(n, p) == -((-1000 * n) // p), (n, p)
    assert lib.bark_hip_tempo_out_len(tr.MAX_SAMPLES, 500) == 2 * tr.MAX_SAMPLES
    for n, p in ((0, 1000), (-1, 1000), (tr.MAX_SAMPLES + 1, 1000), (100, 499), (100, 2001), (100, 0), (100, -1000)):
        assert lib.bark_hip_tempo_out_len(n, p) == -1, (n, p)


def test_window_table_needs_no_context():
    lib = _pkg().load_library()
    w = np.zeros(tr.W, np.float32)
    assert lib.bark_hip_tempo_window(None) == -1 and lib.bark_hip_tempo_window(w.ctypes.data) == tr.W
    assert w.tobytes() == tr.window().tobytes()


def test_entry_points_fail_cleanly_without_a_context():
    lib = _pkg().load_library()
    x = np.zeros(1000, np.float32)
    out = np.zeros(4000, np.float32)
    ints = np.zeros(256, np.int32)
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    n = np.array([1000], np.int32)
    sp = np.array([1250], np.int32)
    assert lib.bark_hip_tempo(None, x.ctypes.data, 1000, 1250, out.ctypes.data, 4000) == -1
    assert lib.bark_hip_tempo_many(None, ptrs, n.ctypes.data, 1, sp.ctypes.data, None, out.ctypes.data, 16000, None) == -1
    assert lib.bark_hip_tempo_positions(None, x.ctypes.data, 1000, 1250, ints.ctypes.data, 256) == -1
    assert lib.bark_hip_get_audio_at(None, None, 1250, out.ctypes.data, 16000) == -1
    assert lib.bark_hip_batch_audio_at(None, 0, None, 1250, out.ctypes.data, 16000) == -1
    assert lib.bark_hip_long_audio_at(None, None, 1250, out.ctypes.data, 16000) == -1
    assert lib.bark_hip_long_audio_at(None, None, 1000, out.ctypes.data, 16000) == -1
    assert lib.bark_hip_time_tempo(None, 8, 1000, 1250, 1) < 0
    assert lib.bark_hip_batcher_submit_at(None, b"a", None, None, None, None, 1250) == -1
    assert lib.bark_hip_batcher_submit_long_at(None, b"a b. c", None, None, None, None, None, 1250) == -1


def test_the_server_speaks_speed():
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    assert '"speed"' in src and '"--speed"' in src and "lround(1000.0 * speed)" in src
    assert "bark_hip_batcher_submit_at(" in src and "bark_hip_batcher_submit_long_at(" in src
