"""The interface of loudness levelling (rule C17l) exists at every layer: exported by libbark.so, declared in include/bark_mi355x.h, mirrored in
bark.cpp_amd/api.py with the declared argument types and struct layouts, spoken by bark_batch_server; and what needs no device: the committed constants and
the target mean square against numpy's evaluation of the formulas, the entry points without a context."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_loudness_constants", "bark_hip_loudness_target_ms", "bark_hip_loudness_many", "bark_hip_loudness_hops", "bark_hip_level_many",
           "bark_hip_get_audio_with", "bark_hip_batch_audio_with", "bark_hip_long_audio_with", "bark_hip_batcher_submit_with", "bark_hip_batcher_submit_long_with",
           "bark_hip_time_loudness"]
METHODS = ["loudness", "loudness_many", "loudness_hops", "level_many", "audio_with", "batch_audio_with", "long_audio_with", "time_loudness"]


def _pkg():
    from bark_amd_loader import load_package
    return load_package()


def _ulps(a, b):
    return abs(float(a) - float(b)) / np.spacing(abs(float(b)))


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
    assert "loudness" not in open(os.path.join(ROOT, "include", "bark.h")).read()


def test_struct_layouts_are_the_header_s():
    pkg = _pkg()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bark_mi355x.h")).read(), flags=re.S)
    assert "struct bark_hip_loudness_params { int32_t target_centilufs; float peak_ceiling; float max_gain; };" in text
    assert "struct bark_hip_loudness_info { double mean_square, lufs; float peak, gain; int32_t n_blocks, n_abs, n_gated, flags; };" in text
    assert "struct bark_hip_audio_render { struct bark_hip_audio_format fmt; int32_t speed_permille; struct bark_hip_loudness_params loudness; };" in text
    P, I, R = pkg.BarkHipLoudnessParams, pkg.BarkHipLoudnessInfo, pkg.BarkHipAudioRender
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("target_centilufs", 0), ("peak_ceiling", 4), ("max_gain", 8)] and C.sizeof(P) == 12
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [("mean_square", 0), ("lufs", 8), ("peak", 16), ("gain", 20), ("n_blocks", 24), ("n_abs", 28),
                                                                  ("n_gated", 32), ("flags", 36)] and C.sizeof(I) == 40
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("fmt", 0), ("speed_permille", 8), ("loudness", 12)] and C.sizeof(R) == 24
    assert (pkg.api.LOUDNESS_UNMEASURABLE, pkg.api.LOUDNESS_CAP_BOUND, pkg.api.LOUDNESS_CEILING_BOUND) == (lr.UNMEASURABLE, lr.CAP_BOUND, lr.CEILING_BOUND) == (1, 2, 4)
    assert "BARK_HIP_LOUDNESS_UNMEASURABLE = 1, BARK_HIP_LOUDNESS_CAP_BOUND = 2, BARK_HIP_LOUDNESS_CEILING_BOUND = 4" in text


def test_methods_are_mirrored_in_python():
    pkg = _pkg()
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    classes = {n.name: {f.name for f in n.body if isinstance(f, ast.FunctionDef)} for n in ast.parse(src).body if isinstance(n, ast.ClassDef)}
    assert [m for m in METHODS if m not in classes["BarkContext"]] == [] and "loudness" in pkg.Batcher.submit.__code__.co_varnames
    p = pkg.loudness_params(-16.0)
    assert (p.target_centilufs, p.peak_ceiling, p.max_gain) == (-1600, 1.0, 10.0)               # the defaults: full scale, +20 dB
    assert [pkg.loudness_params(v).target_centilufs for v in (-40, -23.5, -16.004, -15.996, -5)] == [-4000, -2350, -1600, -1600, -500]
    assert pkg.loudness_params(None).target_centilufs == 0
    r = pkg.audio_render(16000, "s16", 1.25, -23.0)
    assert (r.fmt.sample_rate, r.fmt.sample_format, r.speed_permille, r.loudness.target_centilufs) == (16000, 1, 1250, -2300)


def test_constants_are_the_formulas_to_a_few_ulp_and_need_no_context():
    lib = _pkg().load_library()
    k = np.zeros(9, np.float64)
    assert lib.bark_hip_loudness_constants(None) == -1 and lib.bark_hip_loudness_constants(k.ctypes.data_as(C.POINTER(C.c_double))) == 9
    want = lr.constants()
    for i in range(9):
        assert _ulps(k[i], want[i]) <= 4, (i, k[i], want[i])
    assert k[8] == 9600.0 * k[7]
    src = open(os.path.join(ROOT, "bark.cpp_amd", "csrc", "codec_kernels.hip")).read()
    table = src[src.index("kLoudConst[9] = {"):]
    table = table[:table.index("};")]
    lits = re.findall(r"-?0x1\.[0-9a-f]{13}p[+-]\d+", table)                                    # committed as bit patterns: no libm decides a bit
    assert len(lits) == 9 and [float.fromhex(v) for v in lits] == k.tolist()


def test_target_ms_is_the_formula_to_a_few_ulp_and_refuses_what_it_should():
    lib = _pkg().load_library()
    for t in (-4000, -3999, -2300, -1600, -1401, -501, -500):
        assert _ulps(lib.bark_hip_loudness_target_ms(t), lr.target_ms(t)) <= 4, t
        assert _ulps(lib.bark_hip_loudness_target_ms(t), np.power(10.0, (np.float64(t) / 100.0 + 0.691) / 10.0)) <= 4, t
    for t in (0, -4001, -499, 1600, 2 ** 31 - 1, -2 ** 31):
        assert lib.bark_hip_loudness_target_ms(t) == -1.0, t


def test_entry_points_fail_cleanly_without_a_context():
    pkg = _pkg()
    lib = pkg.load_library()
    x = np.zeros(12000, np.float32)
    out = np.zeros(12000, np.float32)
    z = np.zeros(8, np.float64)
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    n = np.array([12000], np.int32)
    sp = np.array([1000], np.int32)
    par = (pkg.BarkHipLoudnessParams * 1)(pkg.loudness_params(-16.0))
    info = (pkg.BarkHipLoudnessInfo * 1)()
    how = pkg.audio_render(loudness=-16.0)
    assert lib.bark_hip_loudness_many(None, ptrs, n.ctypes.data, 1, par, info) == -1
    assert lib.bark_hip_loudness_hops(None, x.ctypes.data, 12000, z.ctypes.data_as(C.POINTER(C.c_double)), 8) == -1
    assert lib.bark_hip_level_many(None, ptrs, n.ctypes.data, 1, par, sp.ctypes.data, None, out.ctypes.data, 48000, None, info) == -1
    assert lib.bark_hip_get_audio_with(None, C.byref(how), out.ctypes.data, 48000, info) == -1
    assert lib.bark_hip_batch_audio_with(None, 0, C.byref(how), out.ctypes.data, 48000, info) == -1
    assert lib.bark_hip_long_audio_with(None, C.byref(how), out.ctypes.data, 48000, info, 1) == -1
    assert lib.bark_hip_long_audio_with(None, C.byref(pkg.audio_render()), out.ctypes.data, 48000, None, 0) == -1
    assert lib.bark_hip_get_audio_with(None, None, out.ctypes.data, 48000, None) == -1
    assert lib.bark_hip_time_loudness(None, 8, 12000, 0, 1) < 0
    assert lib.bark_hip_batcher_submit_with(None, b"a", None, None, None, C.byref(how)) == -1
    assert lib.bark_hip_batcher_submit_long_with(None, b"a b. c", None, None, None, None, C.byref(how)) == -1


def test_the_server_speaks_loudness():
    src = open(os.path.join(ROOT, "bark.cpp_amd", "examples", "batch_server.cpp")).read()
    assert '"loudness"' in src and '"--loudness"' in src and "lround(100.0 * v)" in src and "1.0f, 10.0f}" in src
    assert "bark_hip_batcher_submit_with(" in src and "bark_hip_batcher_submit_long_with(" in src
    assert src.index('json_number(body, "loudness"') < src.index("next_seed.fetch_add(1)")      # a refused value draws no seed
