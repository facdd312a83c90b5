"""The interface of the FLAC encoder (rule C18f) exists at every layer: exported by libbark.so, declared in include/bark_mi355x.h, mirrored in
bark.cpp_amd/api.py with the declared argument types; one new value of bark_hip_audio_format.sample_format beside the unchanged enum, and no struct changed; bark_hip_flac_max_bytes is the
reference's bound and no frame of the reference passes it; and the argument refusals come before the context is touched.  (A capacity below the real length
needs the encoding: tests/test_gpu_flac.py::test_refusals_leave_the_context_usable checks it, on the host too through tests/test_emulated_flac.py.)"""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import flac_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bark_hip_flac_max_bytes", "bark_hip_flac_encode_many", "bark_hip_flac_frames", "bark_hip_time_flac", "bark_hip_time_flac_launch"]
METHODS = ["flac_encode", "flac_encode_many", "flac_frames", "time_flac"]


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


def test_symbols_are_declared_in_the_header_with_the_mirrored_argument_types():
    pkg = _pkg()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bark_mi355x.h")).read(), flags=re.S)
    lib = pkg.load_library()
    for s in SYMBOLS:
        m = re.search(rf"BARK_API (int|double) {s}\((.*?)\);", text, flags=re.S)
        assert m, s
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        fn = getattr(lib, s)
        assert s in pkg.api.EXPORTS and fn.argtypes is not None and len(fn.argtypes) == len(args), (s, args)
        assert (fn.restype is C.c_double) == (m.group(1) == "double"), s
        for a, t in zip(args, fn.argtypes):
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (s, a)
            else:
                assert a.split()[0] == "int" and t is C.c_int, (s, a)
    assert "flac" not in open(os.path.join(ROOT, "include", "bark.h")).read().lower()


def test_one_new_format_value_and_no_enum_or_struct_changed():
    pkg = _pkg()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bark_mi355x.h")).read(), flags=re.S)
    assert "enum bark_hip_sample_format { BARK_HIP_SAMPLE_F32 = 0, BARK_HIP_SAMPLE_S16 = 1, BARK_HIP_SAMPLE_MULAW = 2 };" in text
    assert "enum bark_hip_container_format { BARK_HIP_SAMPLE_FLAC = 3 };" in text
    assert "struct bark_hip_audio_format { int32_t sample_rate; int32_t sample_format; };" in text
    assert "struct bark_hip_audio_render { struct bark_hip_audio_format fmt; int32_t speed_permille; struct bark_hip_loudness_params loudness; };" in text
    assert C.sizeof(pkg.BarkHipAudioFormat) == 8 and C.sizeof(pkg.BarkHipAudioRender) == 24 and C.sizeof(pkg.BarkHipLoudnessParams) == 12
    assert C.sizeof(pkg.BarkHipLoudnessInfo) == 40 and C.sizeof(pkg.BarkHipJoinParams) == 16 and C.sizeof(pkg.BarkHipLongParams) == 24
    api = pkg.api
    assert (api.SAMPLE_F32, api.SAMPLE_S16, api.SAMPLE_MULAW, api.SAMPLE_FLAC) == (0, 1, 2, 3)
    assert api.SAMPLE_FORMATS == {"f32": 0, "s16": 1, "mulaw": 2} and api.CONTAINER_FORMATS == {"flac": 3}
    assert pkg.audio_format(16000, "flac").sample_format == 3 and pkg.audio_format(16000, "s16").sample_format == 1
    assert api.SAMPLE_DTYPES[api.SAMPLE_FLAC] is np.uint8 and api.FLAC_BLOCK == fr.BLOCK


def test_methods_are_mirrored_in_python():
    pkg = _pkg()
    src = open(os.path.join(ROOT, "bark.cpp_amd", "api.py")).read()
    classes = {n.name: {f.name for f in n.body if isinstance(f, ast.FunctionDef)} for n in ast.parse(src).body if isinstance(n, ast.ClassDef)}
    assert [m for m in METHODS if m not in classes["BarkContext"]] == [] and "audio_format" in pkg.Batcher.submit.__code__.co_varnames
    assert callable(pkg.flac_max_bytes)


def test_max_bytes_is_the_reference_s_bound_and_no_frame_passes_it():
    pkg = _pkg()
    lib = pkg.load_library()
    for n in (1, 2, 4095, 4096, 4097, 8192, 12289, 122880, 1310720, 2 ** 26):
        assert lib.bark_hip_flac_max_bytes(n) == fr.max_bytes(n) == pkg.flac_max_bytes(n), n
    for n in (0, -1, 2 ** 26 + 1, 2 ** 31 - 1, -2 ** 31):
        assert lib.bark_hip_flac_max_bytes(n) == -1, n
    # the worst case: full-scale noise (VERBATIM) under the longest header - three bytes of frame number, the 16-bit block size, the rate in kHz
    rng = np.random.default_rng(9)
    worst, _ = fr.encode_frame(rng.integers(-32768, 32768, 4095), 0x800, 12000)
    assert len(worst) == 14 + 2 * 4095 == lib.bark_hip_flac_max_bytes(4095) - 42 and len(worst) <= fr.FRAME_STRIDE
    for n in (1, 17, 4095, 4096, 4097, 12289):
        for rate in (12000, 24000):
            assert len(fr.encode(fr.signal("white", n), rate)) <= lib.bark_hip_flac_max_bytes(n), (n, rate)
            assert len(fr.encode(fr.signal("alternating", n), rate)) <= lib.bark_hip_flac_max_bytes(n), (n, rate)
    src = open(os.path.join(ROOT, "bark.cpp_amd", "csrc", "kernels.h")).read()
    assert f"kFlacFrameStride = {fr.FRAME_STRIDE};" in src and "kFlacBlock = 4096, kFlacMaxPartitionOrder = 4, kFlacMaxRice = 14" in src


def test_refusals_come_before_the_context_is_touched():
    """a null context, and - with a handle that must not be dereferenced - null arrays, a count outside 1 .. 64, a length below 1 or above 2^26, an unsupported rate"""
    pkg = _pkg()
    lib = pkg.load_library()
    x = fr.signal("sine_click", 4097)
    out = np.zeros(fr.max_bytes(len(x)), np.uint8)
    lengths = np.zeros(65, np.int32)
    rec = np.zeros(8, np.int32)
    fake = C.c_void_p(8)                                                   # every call below is refused on its arguments: the handle is never read

    def many(h, xs, ns, count, rate):
        ptrs = (C.c_void_p * max(len(xs), 1))(*[None if v is None else v.ctypes.data for v in xs])
        n = np.asarray(ns, np.int32)
        return lib.bark_hip_flac_encode_many(h, ptrs, n.ctypes.data, count, rate, out.ctypes.data, out.size, lengths.ctypes.data)
    assert many(None, [x], [len(x)], 1, 24000) == -1
    assert lib.bark_hip_flac_encode_many(fake, None, None, 1, 24000, out.ctypes.data, out.size, None) == -1
    assert lib.bark_hip_flac_encode_many(fake, (C.c_void_p * 1)(x.ctypes.data), None, 1, 24000, out.ctypes.data, out.size, None) == -1
    assert many(fake, [None], [len(x)], 1, 24000) == -1
    assert many(fake, [x], [len(x)], 0, 24000) == -1 and many(fake, [x], [len(x)], -1, 24000) == -1 and many(fake, [x] * 65, [len(x)] * 65, 65, 24000) == -1
    assert many(fake, [x], [0], 1, 24000) == -1 and many(fake, [x], [-5], 1, 24000) == -1 and many(fake, [x], [2 ** 26 + 1], 1, 24000) == -1
    for rate in (0, -1, 11025, 24001, 96000, 192000):
        assert many(fake, [x], [len(x)], 1, rate) == -1, rate
    assert lib.bark_hip_flac_frames(None, x.ctypes.data, len(x), 24000, rec.ctypes.data, 2) == -1
    assert lib.bark_hip_flac_frames(fake, None, len(x), 24000, rec.ctypes.data, 2) == -1
    assert lib.bark_hip_flac_frames(fake, x.ctypes.data, len(x), 24000, None, 2) == -1
    assert lib.bark_hip_flac_frames(fake, x.ctypes.data, len(x), 24000, rec.ctypes.data, 1) == -1            # two frames, room for one record
    assert lib.bark_hip_flac_frames(fake, x.ctypes.data, 0, 24000, rec.ctypes.data, 2) == -1
    assert lib.bark_hip_flac_frames(fake, x.ctypes.data, len(x), 11025, rec.ctypes.data, 2) == -1
    assert lib.bark_hip_time_flac(None, 1, 4096, 1) < 0 and lib.bark_hip_time_flac_launch(None, 1, 4096, 1, 1) < 0
    assert lib.bark_hip_time_flac_launch(fake, 1, 4096, 0, 1) < 0 and lib.bark_hip_time_flac_launch(fake, 1, 4096, 3, 1) < 0
    # the routes that take the format, without a context
    to = pkg.audio_format(16000, "flac")
    how = pkg.audio_render(16000, "flac", 1.25, -16.0)
    assert lib.bark_hip_get_audio_as(None, C.byref(to), out.ctypes.data, out.size) == -1
    assert lib.bark_hip_batch_audio_at(None, 0, C.byref(to), 1250, out.ctypes.data, out.size) == -1
    assert lib.bark_hip_long_audio_with(None, C.byref(how), out.ctypes.data, out.size, None, 0) == -1
    assert lib.bark_hip_batcher_submit_with(None, b"a", None, None, None, C.byref(how)) == -1
